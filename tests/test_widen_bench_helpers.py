"""bench.py end to end at toy sizes (emulated kernels on CPU / the device under -m gpu): the driver's JSON contract for the headline
training line, the multiview C5 workload (--views), the inference line (--predict) and the secondary HBM rooflines."""

import json

import pytest
import torch

import bench

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config")


def _run(capsys, dev, *argv):
    bench.main(list(argv), device=dev)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines  # rank 0 prints ONE JSON line
    out = json.loads(lines[0])
    for key in CONTRACT:
        assert key in out, key
    assert out["n_gpus"] == 1 and out["unit"] == "frames/s" and out["higher_is_better"] is True and out["scaling"] == "weak"
    assert out["vs_baseline"] is None and out["data"] == "synthetic" and out["dtype"] == ("f32" if "fp32" in argv else "bf16")
    assert out["value"] > 0 and out["ms_per_step"] > 0 and "workload" in out["config"]
    return out


def test_bench_training_line(stack_backend, capsys):
    out = _run(capsys, stack_backend, "--steps", "1", "--warmup", "0", "--size", "64", "--labeled", "2", "--unlabeled", "3",
               "--no-cpu-baseline", "--no-profile")
    assert out["metric"].startswith("training frames/sec") and out["steps"] == 1 and out["warmup"] == 0
    assert out["config"]["global_batch"] == 5 and out["config"]["parallelism"] == "dp1"
    assert out["value"] == round(5 * 1 / (out["ms_per_step"] / 1000.0), 2) or abs(out["value"] * out["ms_per_step"] / 1000.0 - 5) < 0.01
    assert torch.isfinite(torch.tensor(out["config"]["final_loss"]))


def test_bench_plain_run_is_lean_and_full_adds_the_extras(stack_backend, capsys):
    """a plain run prints the headline line only; --full adds what takes launches or steps of its own: the idle-queue host step, the
    heat-map HBM rooflines and (on the device, where the HIP events exist) the per-launch MFMA roofline"""
    argv = ("--steps", "3", "--warmup", "0", "--size", "64", "--labeled", "2", "--unlabeled", "3")
    plain = _run(capsys, stack_backend, *argv)
    for key in ("roofline", "roofline_hbm", "cpu_baseline", "secondary", "host_enqueue_idle_queue_ms"):
        assert key not in plain, key
    full = _run(capsys, stack_backend, *argv, "--full", "--no-cpu-baseline")
    assert full["host_enqueue_idle_queue_ms"] > 0 and "cpu_baseline" not in full
    assert set(full["roofline_hbm"]["kernels"]) == {"decode_fwd", "decode_bwd", "heatmap_gen", "heatmap_mse_fwd", "heatmap_mse_bwd"}
    if stack_backend.type == "cuda":
        assert full["roofline"]["sampled_steps"] == 1 and full["roofline"]["launches_per_step"] > 0
    assert full["config"]["comm_per_step"] == plain["config"]["comm_per_step"]


def test_bench_dump_outputs(stack_backend, capsys, tmp_path):
    """--dump-outputs DIR: what the last timed step computed, float32 .npy files within 64 MB, from the same seeded inputs every run"""
    import numpy as np

    argv = ("--steps", "2", "--warmup", "1", "--size", "64", "--labeled", "2", "--unlabeled", "3")
    runs = []
    for name in ("a", "b"):
        out = _run(capsys, stack_backend, *argv, "--dump-outputs", str(tmp_path / name))
        assert out["steps"] == 2
        runs.append({f.stem: np.load(f) for f in sorted((tmp_path / name).glob("*.npy"))})
    a, b = runs
    assert sorted(a) == sorted(b) and {"loss", "logged_total_loss"} <= set(a)
    assert any(k.startswith("params") for k in a) and any(k.startswith("grads") for k in a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert float(a["loss"][0]) == pytest.approx(out["config"]["final_loss"], rel=1e-5, abs=1e-6)
    for k in a:
        assert a[k].dtype == np.float32 and a[k].shape == b[k].shape and np.isfinite(a[k]).all(), k
        if stack_backend.type == "cpu":   # (the emulated kernels are deterministic: the same inputs give the same outputs bit for bit)
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_bench_dump_outputs_predict(stack_backend, capsys, tmp_path):
    import numpy as np

    _run(capsys, stack_backend, "--predict", "--steps", "1", "--warmup", "0", "--size", "64", "--labeled", "2", "--unlabeled", "3",
         "--keypoints", "3", "--dump-outputs", str(tmp_path))
    kp, conf = np.load(tmp_path / "keypoints.npy"), np.load(tmp_path / "confidences.npy")
    assert kp.shape == (5, 6) and conf.shape == (5, 3) and kp.dtype == np.float32 and np.isfinite(kp).all()


def test_bench_fp32_line(stack_backend, capsys):
    """the secondary line at the reference's own precision (VERDICT r4 "missing" 4): the same step on the fp32 validation executor"""
    out = _run(capsys, stack_backend, "--steps", "1", "--warmup", "0", "--size", "64", "--labeled", "2", "--unlabeled", "3",
               "--no-cpu-baseline", "--no-profile", "--precision", "fp32")
    assert "fp32" in out["config"]["workload"] and "mfma_frac_end_to_end" not in out
    assert torch.isfinite(torch.tensor(out["config"]["final_loss"]))


def test_bench_multiview_line(stack_backend, capsys):
    out = _run(capsys, stack_backend, "--steps", "1", "--warmup", "0", "--size", "32", "--labeled", "1", "--unlabeled", "3", "--views", "2",
               "--keypoints", "3", "--no-cpu-baseline", "--no-profile")
    assert out["config"]["workload"].startswith("C5: multiview") and out["config"]["global_batch"] == (1 + 3) * 2


def test_bench_predict_line(stack_backend, capsys):
    out = _run(capsys, stack_backend, "--predict", "--steps", "1", "--warmup", "0", "--size", "64", "--labeled", "2", "--unlabeled", "3",
               "--keypoints", "3")
    assert out["metric"].startswith("inference frames/sec") and out["config"]["global_batch"] == 5 and out["config"]["finite"] is True


def test_bench_fit_line(stack_backend, capsys):
    """--fit: Trainer.fit over FrameWindowSource / VideoFramePipeline / LabeledBatchProducer (uint8 host frames in, the step out); the
    logged scalars reach the host once (end of the epoch), not per step"""
    out = _run(capsys, stack_backend, "--fit", "--steps", "1", "--warmup", "0", "--size", "128", "--labeled", "1", "--unlabeled", "2",
               "--keypoints", "3", "--no-cpu-baseline", "--no-profile")
    assert out["metric"].startswith("training frames/sec through Trainer.fit") and out["config"]["host_records"] == 1
    assert torch.isfinite(torch.tensor(out["config"]["final_loss"]))


def test_cpu_baseline_is_the_reference_itself_when_its_modules_are_there():
    """bench.py's cpu_baseline leg times the reference's OWN tracker step (kind "reference": /root/reference, or oracle/_ref on the GPU
    box) and falls back to the restated port (kind "port") only when neither tree exists"""
    from oracle import ref_loader as R

    if not R.available():
        pytest.skip("neither /root/reference nor oracle/_ref present")
    out = bench.cpu_baseline_reference(64, 17, n_lab=2, n_unlab=3, steps=1)
    assert out["kind"] == "reference" and out["value"] > 0 and out["unit"] == "frames/s" and "verbatim" in out["sample"]


def test_hbm_rooflines_runs_the_heatmap_kernels(stack_backend):
    out = bench.hbm_rooflines(stack_backend, 64, 3, 4, reps=1)
    assert out["bound"] == "hbm" and out["algorithmic_bytes_per_frame"] == 3 * 16 * 16 * 4
    assert set(out["kernels"]) == {"decode_fwd", "decode_bwd", "heatmap_gen", "heatmap_mse_fwd", "heatmap_mse_bwd"}
    assert "valu_frac" in out["kernels"]["decode_fwd"] and "C-ABI" in out["timed"]
    for v in out["kernels"].values():
        assert v["us"] > 0 and v["achieved"] >= 0  # (the emulator moves kilobytes per millisecond)


def test_bench_two_ranks_gloo():
    """`bench.py --gpus 2` as the driver launches it (one process per rank, env rendezvous on 127.0.0.1), on CPU: gloo backend, emulated
    kernels.  Rank 0 prints ONE line whose value is the whole-job rate; SyncBatchNorm and the gradient all-reduce are on."""
    import os
    import socket
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    argv = ["--gpus", "2", "--steps", "1", "--warmup", "0", "--size", "32", "--labeled", "2", "--unlabeled", "2", "--keypoints", "3",
            "--no-cpu-baseline", "--no-profile"]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   LP_DIST_BACKEND="gloo", HIPEMU_THREADS="4")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "_bench_2rank_probe.py"), *argv], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=900) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-1500:] for o in outs]
    lines0 = [ln for ln in outs[0][0].splitlines() if ln.startswith("{")]
    lines1 = [ln for ln in outs[1][0].splitlines() if ln.startswith("{")]
    assert len(lines0) == 1 and lines1 == []  # only rank 0 reports
    out = json.loads(lines0[0])
    for key in CONTRACT:
        assert key in out, key
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 8 and out["config"]["parallelism"] == "dp2"
    assert out["config"]["sync_batchnorm"] is True and out["scaling"] == "weak" and out["value"] > 0
    assert "cpu_baseline" not in out  # rank 0 at N = 1 only


def test_bench_self_launches_its_ranks():
    """`python bench.py --gpus 2` typed WITHOUT a launcher (no WORLD_SIZE in the environment) spawns its own two ranks through
    torch.distributed.run on 127.0.0.1 - here each rank is the CPU probe (gloo + emulated kernels); rank 0's line is the only JSON line."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = ["--gpus", "2", "--steps", "1", "--warmup", "0", "--size", "32", "--labeled", "2", "--unlabeled", "2", "--keypoints", "3",
            "--no-cpu-baseline", "--no-profile"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(LP_DIST_BACKEND="gloo", HIPEMU_THREADS="4")
    code = ("import sys; sys.path.insert(0, %r); import bench; "
            "raise SystemExit(bench.self_launch(2, %r, entry=%r))" % (root, argv, os.path.join(root, "tests", "_bench_2rank_probe.py")))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "dp2" and out["config"]["sync_batchnorm"] is True and out["value"] > 0
    assert out["config"]["comm_per_step"]["grad_buckets"] >= 1


def test_bench_main_hands_over_to_self_launch_without_a_launcher(monkeypatch):
    """main(--gpus N) with no WORLD_SIZE calls self_launch with the same argv and exits with its code; with WORLD_SIZE set (a launcher is
    around us) or --gpus 1 it never does."""
    calls = []
    monkeypatch.setattr(bench, "self_launch", lambda n, argv, **kw: calls.append((n, list(argv))) or 7)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "4", "--steps", "3"])
    assert e.value.code == 7 and calls == [(4, ["--gpus", "4", "--steps", "3"])]
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:   # a launcher with the wrong world size is still an error, not a second launch
        bench.main(["--gpus", "4", "--steps", "3"], device=torch.device("cpu"))
    assert "WORLD_SIZE=2" in str(e.value.code) and len(calls) == 1


def test_bench_gpus_8_launcher_command(monkeypatch, capsys):
    """`python bench.py --gpus 8 --syncbn-gather` with no launcher around it (what the driver's SCALE run may type): the command it would run -
    torch.distributed.run, one node, 8 processes, rendezvous on 127.0.0.1, this script with the same flags - and the environment of its
    ranks (dmabuf IPC for RCCL, a thread budget per rank, the SyncBatchNorm transport), checked without starting anything"""
    import os
    import sys

    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LP_SYNCBN_GATHER", "OMP_NUM_THREADS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LP_BENCH_DRY_RUN", "1")
    argv = ["--gpus", "8", "--steps", "20", "--warmup", "3", "--syncbn-gather"]
    with pytest.raises(SystemExit) as e:
        bench.main(argv)
    assert e.value.code == 0
    rec = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    cmd = rec["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nnodes=1" in cmd and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-len(argv) - 1:] == [os.path.abspath(bench.__file__)] + argv
    assert rec["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and rec["env"]["LP_SYNCBN_GATHER"] == "1"
    assert int(rec["env"]["OMP_NUM_THREADS"]) == max(1, (os.cpu_count() or 8) // 8)
    monkeypatch.delenv("LP_SYNCBN_GATHER", raising=False)


def _free_port() -> int:
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


LOOPBACK_ARGV = ["--gpus", "1", "--steps", "1", "--warmup", "1", "--size", "32", "--labeled", "2", "--unlabeled", "2", "--keypoints", "3", "--no-cpu-baseline",
                 "--no-profile", "--no-secondary"]


def _check_loopback_line(stdout: str, backend: str) -> dict:
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    comm = out["config"]["comm_per_step"]
    assert out["n_gpus"] == 1 and out["config"]["sync_batchnorm"] is True and comm["backend"] == backend
    assert comm["sync_bn_messages"] > 0 and comm["grad_buckets"] >= 1 and comm["logged_scalar_messages"] == 1
    assert out["value"] > 0 and out["config"]["final_loss"] == out["config"]["final_loss"]  # finite
    return out


def test_bench_loopback_gloo():
    """LP_DIST_LOOPBACK=1: every collective of the step is issued on a world of one rank (here gloo + emulated kernels).  The SyncBatchNorm
    messages per step are the same whether or not --full adds its untimed idle-queue step: the count is divided by the steps that ran."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = []
    for extra in ([], ["--full"]):
        env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
                   LP_DIST_BACKEND="gloo", LP_DIST_LOOPBACK="1", HIPEMU_THREADS="4")
        p = subprocess.run([sys.executable, os.path.join(root, "tests", "_bench_2rank_probe.py"), *LOOPBACK_ARGV, *extra], env=env,
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        lines.append(_check_loopback_line(p.stdout, "gloo"))
    plain, full = (ln["config"]["comm_per_step"] for ln in lines)
    assert "host_enqueue_idle_queue_ms" in lines[1] and "host_enqueue_idle_queue_ms" not in lines[0]
    assert plain["sync_bn_messages"] == full["sync_bn_messages"], (plain, full)


@pytest.mark.gpu
def test_bench_loopback_rccl_on_device():
    """The same on the device over RCCL (backend "nccl"): communicator bound to the rank's GPU, gradient buckets handed from the
    weight-gradient side stream to RCCL's stream during backward, SyncBatchNorm messages between kernels of one stream, the packed scalar
    message - the stream semantics the gloo tests cannot see.  One rank is all a single-GPU box offers; the arithmetic is the N = 1 step's."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               LP_DIST_LOOPBACK="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("LP_DIST_BACKEND", None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *LOOPBACK_ARGV], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out = _check_loopback_line(p.stdout, "nccl")
    assert out["config"]["comm_per_step"]["sync_bn_transport"] == "all_reduce"
    # ... and with the SyncBatchNorm messages as the one-shot exchange (RCCL all-gather into per-rank slots + local add in rank order)
    env.update(LP_SYNCBN_GATHER="1", MASTER_PORT=str(_free_port()))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *LOOPBACK_ARGV], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    gather = _check_loopback_line(p.stdout, "nccl")
    assert gather["config"]["comm_per_step"]["sync_bn_transport"].startswith("all_gather")
    assert gather["config"]["final_loss"] == pytest.approx(out["config"]["final_loss"], rel=1e-3)   # sums over one rank: the same step


def test_smoke_entry_point_body(stack_backend, capsys):
    """__graft_entry__.smoke() - the driver's round-end tier - runs its own body here (emulated kernels on CPU; the device under -m gpu)"""
    import __graft_entry__ as entry

    entry.smoke(device=stack_backend)
    assert "smoke ok" in capsys.readouterr().out
