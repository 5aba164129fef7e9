"""DINOv3 mode of the ViT engine (``ViTEngine(arch="dinov3")`` / ``Fp32ViTEngine``) against the installed ``transformers.DINOv3ViTModel`` built
from a ``DINOv3ViTConfig`` (never ``from_pretrained``), in float64 on the CPU, wrapped as the reference's ``VisionEncoderDino.forward`` does
(models/backbones/vit_dino.py: drop [CLS] and the register tokens, reshape to (B, D, gh, gw)) and followed by the PixelShuffle /
ConvTranspose2d head and the soft-max.  Heat-maps and EVERY parameter gradient - ``register_tokens``, ``cls_token``, both ``lambda1`` of every
layer, ``q_proj.bias`` - at the bars tests/test_dinov2_engine.py applies to the same comparisons; the training-mode coordinate augmentation is
checked by replaying the engine's own per-part draws in the HF model."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

transformers = pytest.importorskip("transformers")

PRE = "backbone.vision_encoder."
SMALL = (128, 2, 2, 256, 4)       # hidden, depth, heads, mlp, register tokens
HEAD_KEYS = {"head.upsampling_layers.1.weight", "head.upsampling_layers.1.bias"}


def _config(hidden, depth, heads, mlp, registers, **kw):
    from transformers import DINOv3ViTConfig
    cfg = DINOv3ViTConfig(hidden_size=hidden, num_hidden_layers=depth, num_attention_heads=heads, intermediate_size=mlp,
                          num_register_tokens=registers, image_size=48, patch_size=16, **kw)
    assert cfg.layer_norm_eps == 1e-5 and not cfg.use_gated_mlp and not cfg.key_bias and cfg.rope_theta == 100.0
    assert cfg.drop_path_rate == 0.0 and cfg.attention_dropout == 0.0      # .train() changes the coordinates only
    return cfg


def _oracle(K, hidden, depth, heads, mlp, registers, seed, **kw):
    from transformers import DINOv3ViTModel
    torch.manual_seed(seed)
    vit = DINOv3ViTModel(_config(hidden, depth, heads, mlp, registers, **kw)).eval()
    with torch.no_grad():  # make every parameter non-trivial (HF initialises biases / LayerNorm / lambda1 to 0 / 1 / 1)
        for n, p in vit.named_parameters():
            if n.endswith("lambda1"):   # away from 1 and of both signs: with lambda1 = 1 a missing scale is invisible
                p.copy_((0.2 + 1.3 * torch.rand_like(p)) * (torch.randint(0, 2, p.shape) * 2 - 1))
            elif p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        vit.embeddings.cls_token.normal_(std=0.5)
        vit.embeddings.register_tokens.normal_(std=0.5)
    head = nn.Sequential(nn.PixelShuffle(2), nn.ConvTranspose2d(hidden // 4, K, 3, 2, 1, 1))
    with torch.no_grad():
        head[1].weight.normal_(std=0.3)
        head[1].bias.normal_(std=0.1)
    return vit.double(), head.double()


def _oracle_forward(vit, head, images):
    R = vit.config.num_register_tokens
    hs = vit(images.double()).last_hidden_state[:, 1 + R:]
    b, _, hh, ww = images.shape
    feat = hs.reshape(b, hh // 16, ww // 16, -1).permute(0, 3, 1, 2)
    logits = head(feat)
    b, k, h, w = logits.shape
    return torch.softmax(logits.reshape(b, k, -1), -1).reshape(b, k, h, w)


def _state(vit, head):
    sd = {PRE + k: v.detach().float() for k, v in vit.state_dict().items()}
    sd["head.upsampling_layers.1.weight"] = head[1].weight.detach().float()
    sd["head.upsampling_layers.1.bias"] = head[1].bias.detach().float()
    return sd


def _engine(dev, K, cfg, fp32, vit, head, **kw):
    from lightning_pose_amd.vit_engine import ViTEngine
    if fp32:
        from lightning_pose_amd.vit_engine_fp32 import Fp32ViTEngine as ViTEngine  # noqa: F811
    hidden, depth, heads, mlp, registers = cfg
    eng = ViTEngine(K, 2, dev, hidden=hidden, depth=depth, heads=heads, mlp=mlp, patch=16, arch="dinov3", registers=registers, **kw)
    assert eng.ln_eps == 1e-5 and eng.plan.n_pos == 0 and eng.n_prefix == 1 + registers
    eng.load_state_dict(_state(vit, head), strict=True)
    return eng


def _compare(heat, want, grads, ref, hidden, fp32, tag):
    """the bars of tests/test_dinov2_engine.py; every figure is printed before it is asserted"""
    err = (heat - want).abs()
    print(f"[{tag}] heat-maps: max abs err {err.max().item():.3e}, max err / (atol + rtol |want|) "
          f"{(err / ((1e-6 + 1e-4 * want.abs()) if fp32 else (2e-3 + (5e-2 if hidden == 128 else 1e-1) * want.abs()))).max().item():.3f}")
    if fp32:
        torch.testing.assert_close(heat, want, atol=1e-6, rtol=1e-4)
    else:
        torch.testing.assert_close(heat, want, atol=2e-3, rtol=5e-2 if hidden == 128 else 1e-1)   # (the DINOv2 file's bar per width)
    assert set(grads) == set(ref)                             # (no k_proj.bias on either side)
    assert not any(k.endswith("k_proj.bias") for k in grads)
    mask = PRE + "embeddings.mask_token"
    assert not grads[mask].any() and not ref[mask].any()      # the forward pass never reads it: exactly zero
    worst = (1.0, 0.0, "")
    seen = 0
    for k, gr in ref.items():
        got = grads[k].reshape(gr.shape)
        if gr.norm() < 1e-5:
            # analytically zero (the soft-max over pixels is invariant to the head's per-channel bias; mask_token): only rounding noise
            assert k == mask or k == "head.upsampling_layers.1.bias", k
            assert got.norm() < (1e-5 if fp32 else 5e-3), (k, got.norm().item())
            continue
        cos = F.cosine_similarity(got.flatten(), gr.flatten(), dim=0).item()
        rel = ((got - gr).norm() / gr.norm()).item()
        if rel > worst[1]:
            worst = (cos, rel, k)
        if k.endswith(("lambda1", "cls_token", "register_tokens", "q_proj.bias")):
            seen += 1
            print(f"[{tag}] {k}: cos {cos:.6f} rel {rel:.3e}")
        if fp32:
            assert rel < 1e-4, (k, cos, rel)
        else:
            assert cos > 0.999 and rel < 0.03, (k, cos, rel)
    print(f"[{tag}] worst gradient: {worst[2]} cos {worst[0]:.6f} rel {worst[1]:.3e}")
    return seen


def _grads_and_ref(eng, vit, head):
    grads = {k: v.detach().cpu().clone() for k, v in eng.grad_views().items()}
    ref = {PRE + k: (p.grad if p.grad is not None else torch.zeros_like(p)).float() for k, p in vit.named_parameters()}
    ref["head.upsampling_layers.1.weight"] = head[1].weight.grad.float()
    ref["head.upsampling_layers.1.bias"] = head[1].bias.grad.float()
    return grads, ref


def check_dinov3_engine_vs_hf(dev, cfg, B, H, W, fp32, parts=None, tag=""):
    K = 5
    vit, head = _oracle(K, *cfg, seed=0)
    eng = _engine(dev, K, cfg, fp32, vit, head)
    gen = torch.Generator().manual_seed(1)
    images = torch.randn(B, 3, H, W, generator=gen)
    # eval mode on both sides: the plain coordinates (the training-mode draws have their own test below)
    if parts is None:
        heat, tape = eng.forward(images.to(dev), False)
    else:   # a joint pass of two batches
        assert sum(parts) == B
        heat, tape = eng.forward((images[:parts[0]].to(dev), images[parts[0]:].to(dev)), False)
    assert tape.meta["rope"] is None
    want = _oracle_forward(vit, head, images)
    assert heat.shape == want.shape == (B, K, H // 4, W // 4)
    g = torch.randn(want.shape, generator=gen)
    (want * g.double()).sum().backward()
    eng.zero_grad()
    eng.backward(tape, g.to(dev))
    grads, ref = _grads_and_ref(eng, vit, head)
    seen = _compare(heat.cpu(), want.detach().float(), grads, ref, cfg[0], fp32, tag or f"B{B} {H}x{W} {'fp32' if fp32 else 'bf16'}")
    assert seen == 3 * cfg[1] + 2     # both lambda1 and q_proj.bias of every layer, cls_token and register_tokens: compared, not skipped as zero
    return eng, images, heat


# 48 x 64: a 3 x 4 grid (a y / x swap of the rotary angles shows);  32 x 48: 2 x 3
@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,W", [(48, 64), (32, 48)])
def test_dinov3_engine_forward_backward_vs_hf(stack_backend, H, W, fp32):
    check_dinov3_engine_vs_hf(stack_backend, SMALL, 3, H, W, fp32)


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_dinov3_engine_joint_pass_of_two_batches(stack_backend, fp32):
    """labeled + unlabeled frames in one pass (2 + 1 images) against the oracle's single pass, and equal to the engine's own single pass"""
    dev = stack_backend
    eng, images, heat = check_dinov3_engine_vs_hf(dev, SMALL, 3, 32, 48, fp32, parts=(2, 1))
    assert eng.can_segment(2, 32, 48)
    single, _ = eng.forward(images.to(dev), False)
    assert torch.equal(single, heat)


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("knobs", [dict(pos_embed_rescale=2.0), dict(pos_embed_shift=0.3, pos_embed_jitter=1.5, pos_embed_rescale=2.0)],
                         ids=["rescale", "shift+jitter+rescale"])
def test_dinov3_training_mode_draws_replayed_in_hf(stack_backend, fp32, knobs, monkeypatch):
    """training=True, parts=(2, 1): one draw per part, taken from tape.meta["rope"] and applied by the HF model in .train() - one call per
    part, as the reference's labeled and unlabeled forward passes are"""
    from transformers.models.dinov3_vit import modeling_dinov3_vit as M
    dev, K = stack_backend, 5
    vit, head = _oracle(K, *SMALL, seed=0, **{k: v for k, v in knobs.items()})
    eng = _engine(dev, K, SMALL, fp32, vit, head, rope_seed=3, **{"pos_embed_shift": None, "pos_embed_jitter": None, **knobs})
    gen = torch.Generator().manual_seed(1)
    images = torch.randn(3, 3, 48, 64, generator=gen)
    pair = (images[:2].to(dev), images[2:].to(dev))
    heat, tape = eng.forward(pair, True)
    draws = tape.meta["rope"]
    assert len(draws) == 2 and all(set(d) == {k[len("pos_embed_"):] for k in knobs} for d in draws)
    assert not torch.equal(draws[0]["rescale"], draws[1]["rescale"])             # each part has its own draw
    assert all(0.5 <= float(d["rescale"]) <= 2.0 for d in draws)

    current = {}

    def replay(coords, shift=None, jitter=None, rescale=None):
        d = current["draw"]
        assert (shift is None) == ("shift" not in d) and (jitter is None) == ("jitter" not in d) and (rescale is None) == ("rescale" not in d)
        if "shift" in d:
            coords = coords + d["shift"]
        if "jitter" in d:
            coords = coords * d["jitter"]
        if "rescale" in d:
            coords = coords * d["rescale"]
        return coords

    monkeypatch.setattr(M, "augment_patches_center_coordinates", replay)
    vit.train()
    outs = []
    for d, part in zip(draws, (images[:2], images[2:])):
        current["draw"] = d
        outs.append(_oracle_forward(vit, head, part))
    want = torch.cat(outs)
    g = torch.randn(want.shape, generator=gen)
    (want * g.double()).sum().backward()
    eng.zero_grad()
    eng.backward(tape, g.to(dev))
    grads, ref = _grads_and_ref(eng, vit, head)
    _compare(heat.cpu(), want.detach().float(), grads, ref, SMALL[0], fp32, f"train {'+'.join(knobs)} {'fp32' if fp32 else 'bf16'}")

    heat2, tape2 = eng.forward(pair, True)                                          # a second forward draws anew
    assert not torch.equal(tape2.meta["rope"][0]["rescale"], draws[0]["rescale"]) and not torch.equal(heat2, heat)
    heat3, tape3 = eng.forward(pair, True, rope=draws)                              # ... and rope= replays the same bits
    assert torch.equal(heat3, heat) and tape3.meta["rope"][1]["rescale"] is draws[1]["rescale"]
    plain, tape4 = eng.forward(pair, False)                                         # training=False ignores the knobs
    assert tape4.meta["rope"] is None and not torch.equal(plain, heat)
    vit.eval()
    with torch.no_grad():
        want_plain = _oracle_forward(vit, head, images).float()
    torch.testing.assert_close(plain.cpu(), want_plain, atol=1e-6 if fp32 else 2e-3, rtol=1e-4 if fp32 else 5e-2)
    assert torch.equal(eng.forward_infer(images.to(dev)), eng.forward(images.to(dev), False)[0])


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_dinov3_state_dict_names_and_strict_load_both_ways(stack_backend, fp32):
    dev = stack_backend
    vit, head = _oracle(5, *SMALL, seed=0)
    eng = _engine(dev, 5, SMALL, fp32, vit, head)
    own = eng.state_dict()
    want = {PRE + k for k in vit.state_dict()} | HEAD_KEYS
    assert set(own) == want == set(eng.grad_views())
    assert set(eng.grad_views()) == {PRE + n for n, _ in vit.named_parameters()} | HEAD_KEYS
    sd = _state(vit, head)
    for k, v in own.items():                                                   # HF -> engine: every tensor arrived, bit for bit
        assert torch.equal(v.cpu(), sd[k].reshape(v.shape)), k
    assert own[PRE + "embeddings.register_tokens"].shape == (1, 4, 128) and own[PRE + "embeddings.mask_token"].shape == (1, 1, 128)
    assert own[PRE + "embeddings.patch_embeddings.weight"].shape == (128, 3, 16, 16)
    q, kk, v = (own[PRE + f"model.layer.0.attention.{n}_proj.weight"] for n in "qkv")
    assert kk.data_ptr() - q.data_ptr() == 128 * 128 * 4 == v.data_ptr() - kk.data_ptr()       # q / k / v: views of ONE fused GEMM weight
    from transformers import DINOv3ViTModel
    fresh = DINOv3ViTModel(vit.config)
    fresh.load_state_dict({k[len(PRE):]: v.cpu() for k, v in own.items() if k.startswith(PRE)}, strict=True)      # engine -> HF
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[PRE + k]), k
    with pytest.raises(KeyError):
        eng.load_state_dict({k: v for k, v in sd.items() if not k.endswith("register_tokens")}, strict=True)
    with pytest.raises(KeyError, match="k_proj.bias"):
        eng.load_state_dict({**sd, PRE + "model.layer.0.attention.k_proj.bias": torch.zeros(128)}, strict=True)
    # a fresh engine: lambda1 = 1, mask_token = 0, every backbone tensor inside the backbone's optimiser range
    from lightning_pose_amd.vit_engine import ViTEngine
    new = ViTEngine(5, 2, dev, hidden=128, depth=2, heads=2, mlp=256, patch=16, arch="dinov3")
    assert new.plan.registers == 4 and new.rope_aug == dict(shift=None, jitter=None, rescale=2.0) and new.rope_theta == 100.0
    fresh_sd = new.state_dict()
    assert torch.equal(fresh_sd[PRE + "model.layer.0.layer_scale1.lambda1"].cpu(), torch.ones(128))
    assert not fresh_sd[PRE + "embeddings.mask_token"].any()
    lo, hi = new.plan.group_ranges()["backbone"]
    for k, v in fresh_sd.items():
        off = (v.data_ptr() - new.P.data_ptr()) // 4
        assert (lo <= off and off + v.numel() <= hi) == k.startswith(PRE), k


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_dinov3_inference_forward_equals_eval_forward(stack_backend, fp32):
    dev = stack_backend
    vit, head = _oracle(5, *SMALL, seed=0)
    eng = _engine(dev, 5, SMALL, fp32, vit, head)
    images = torch.randn(3, 3, 32, 48, generator=torch.Generator().manual_seed(2)).to(dev)
    heat, _ = eng.forward(images, False)
    assert torch.equal(eng.forward_infer(images), heat)


def _key_slots(eng):
    D = eng.plan.D
    return [(L["qkv"].b_off + D, L["qkv"].b_off + 2 * D) for L in eng.plan.layers]


def test_dinov3_grad_progress_announces_only_final_tails(stack_backend):
    """the LayerScale gradients are written by the NEXT LayerNorm backward, and the key third of the fused bias gradient is cleared before its
    layer is announced: every tail of G announced during the backward pass is final"""
    dev = stack_backend
    vit, head = _oracle(5, *SMALL, seed=0)
    eng = _engine(dev, 5, SMALL, False, vit, head)
    snaps = []
    eng.grad_progress = lambda off: snaps.append((off, eng.G[off:].detach().cpu().clone()))
    eng.single_backward = True
    images = torch.randn(2, 3, 32, 48, generator=torch.Generator().manual_seed(3)).to(dev)
    heat, tape = eng.forward(images, True)
    eng.zero_grad()
    eng.backward(tape, torch.randn(heat.shape, generator=torch.Generator().manual_seed(4)).to(dev))
    final = eng.G.detach().cpu().clone()
    assert len(snaps) == 1 + SMALL[1]
    for off, snap in snaps:
        assert torch.equal(snap, final[off:]), off
    for lo, hi in _key_slots(eng):
        assert not final[lo:hi].any()


@pytest.mark.parametrize("precision", ["bf16-mixed", "fp32"])
def test_dinov3_key_bias_slot_stays_zero_under_fused_adam(stack_backend, precision, monkeypatch):
    """three FusedAdam steps with weight decay on the tracker's groups: the key third of every fused bias vector is exactly 0 in P afterwards,
    and its slice of G exactly 0 after every backward pass"""
    from lightning_pose_amd import ops
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import get_model_class
    from lightning_pose_amd.models.backbones import factory as bf
    from lightning_pose_amd.optim import FusedAdam
    from lightning_pose_amd.trainer import Trainer

    dev = stack_backend
    monkeypatch.setitem(bf.DINOV3_CONFIGS, "vits_dinov3", (128, 2, 2, 256, 16, 4))
    model = get_model_class("heatmap", False)(
        num_keypoints=3, loss_factory=LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None), backbone="vits_dinov3", pretrained=False,
        torch_seed=0, device=dev, optimizer="AdamW", optimizer_params={"learning_rate": 1e-3}, precision=precision)   # (AdamW: decoupled weight decay 0.01)
    eng = model.net
    with torch.no_grad():   # biases away from zero: the rotated key bias that is NOT there would show in the column sums
        for k, v in eng.state_dict().items():
            if k.endswith(".bias") and k.startswith(PRE):
                v.normal_(std=0.3, generator=None)
    eng.refresh_weight_copies()
    gen = torch.Generator().manual_seed(0)
    kp = torch.rand(2, 3, 2, generator=gen) * 60 + 2
    batch = {"images": torch.randn(2, 3, 64, 64, generator=gen).to(dev), "keypoints": kp.reshape(2, -1).to(dev),
             "heatmaps": ops.generate_heatmaps(kp.to(dev), 64, 64, (16, 16)), "bbox": torch.tensor([[0.0, 0.0, 64.0, 64.0]] * 2).to(dev)}
    tr = Trainer(data_parallel=False)
    tr.setup(model)
    opt = model.optimizers()
    assert isinstance(opt, FusedAdam)
    for g in opt.param_groups:
        g["lr"] = 1e-3
    model.train()
    seen = []
    real_backward = eng.backward

    def backward(tape, g_heat, trace=None):
        real_backward(tape, g_heat, trace)
        seen.append([eng.G[lo:hi].detach().cpu().clone() for lo, hi in _key_slots(eng)])
        # the weight-gradient pass DID leave non-zero column sums next to the slot (the query and value thirds)
        assert all(eng.G[lo - eng.plan.D:lo].any() and eng.G[hi:hi + eng.plan.D].any() for lo, hi in _key_slots(eng))

    monkeypatch.setattr(eng, "backward", backward)
    before = eng.P.detach().cpu().clone()
    for i in range(3):
        tr.training_batch(model, batch, i)
    assert len(seen) == 3 and all(not s.any() for step in seen for s in step)
    after = eng.P.detach().cpu()
    assert not torch.equal(after, before)
    for lo, hi in _key_slots(eng):
        assert not after[lo:hi].any()
    assert not any(k.endswith("k_proj.bias") for k in model.state_dict())


def test_dinov3_bias_and_gelu_switches_agree(stack_backend, monkeypatch):
    """LP_VIT_BIAS_FUSED=0 / LP_VIT_GELU_FUSED=0 select the prefix-dropping LayerScale walk without column sums: the same gradients up to the
    summation order of the bias gradients"""
    dev = stack_backend
    vit, head = _oracle(5, *SMALL, seed=0)

    def grads(bias, gelu):
        monkeypatch.setenv("LP_VIT_BIAS_FUSED", bias)
        monkeypatch.setenv("LP_VIT_GELU_FUSED", gelu)
        eng = _engine(dev, 5, SMALL, False, vit, head)
        images = torch.randn(2, 3, 48, 48, generator=torch.Generator().manual_seed(5)).to(dev)
        heat, tape = eng.forward(images, False)
        eng.zero_grad()
        eng.backward(tape, (torch.randn(heat.shape, generator=torch.Generator().manual_seed(6)).to(dev)) * heat)
        return {k: v.detach().cpu().clone() for k, v in eng.grad_views().items()}

    a = grads("1", "1")
    for bias, gelu in (("0", "1"), ("1", "0")):
        b = grads(bias, gelu)
        for k in a:
            if k.endswith("lambda1") or a[k].dim() > 1 and "upsampling" not in k:
                scale = float(a[k].abs().max())
                assert scale > 0 or "mask_token" in k, k
                torch.testing.assert_close(a[k], b[k], atol=1e-5 * scale, rtol=0, msg=k)


def test_dinov3_refuses_what_is_out_of_scope(stack_backend):
    from lightning_pose_amd.vit_engine import ViTEngine
    from lightning_pose_amd.vit_engine_fp32 import Fp32ViTEngine
    kw = dict(hidden=128, depth=2, heads=2, mlp=256, patch=16)
    for cls in (ViTEngine, Fp32ViTEngine):
        with pytest.raises(NotImplementedError, match="multi-view"):
            cls(5, 2, stack_backend, num_views=4, arch="dinov3", **kw)
        with pytest.raises(ValueError, match="pretrain_grid"):       # there is no position table to size
            cls(5, 2, stack_backend, pretrain_grid=3, arch="dinov3", **kw)
        with pytest.raises(ValueError, match="registers"):
            cls(5, 2, stack_backend, arch="dinov2", registers=4, **kw)
    eng = ViTEngine(5, 2, stack_backend, arch="dinov3", registers=0, **kw)       # R = 0: [CLS] alone in front of the patches
    heat, _ = eng.forward(torch.randn(1, 3, 32, 32).to(stack_backend), False)
    assert heat.shape == (1, 5, 8, 8) and torch.isfinite(heat).all() and PRE + "embeddings.register_tokens" in eng.state_dict()


@pytest.mark.gpu
@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hidden,heads", [(384, 6), (768, 12)])
def test_dinov3_engine_full_width_vs_hf(hidden, heads, fp32):
    """the real widths (NP = 3 and NP = 6 of the LayerNorm walks, 6 and 12 heads under the rotation), depth 2, on the device"""
    check_dinov3_engine_vs_hf(torch.device("cuda:0"), (hidden, 2, heads, 4 * hidden, 4), 2, 32, 32, fp32)
