"""DINOv2 mode of the ViT engine (``ViTEngine(arch="dinov2")`` / ``Fp32ViTEngine``) against the installed ``transformers.Dinov2Model`` built from
a ``Dinov2Config`` (never ``from_pretrained``), in float64 on the CPU, wrapped as the reference's ``VisionEncoderDino.forward`` does
(models/backbones/vit_dino.py: drop [CLS], reshape to (B, D, gh, gw)) and followed by the PixelShuffle / ConvTranspose2d head and the soft-max.
Heat-maps and EVERY parameter gradient - both ``lambda1`` of every layer, ``cls_token``, ``position_embeddings`` - at the bars
tests/test_mvt_engine.py applies to the same comparisons."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

transformers = pytest.importorskip("transformers")

PRE = "backbone.vision_encoder."
SMALL = (128, 2, 2, 2, 3)       # hidden, depth, heads, mlp ratio, pretraining grid (image_size 48 at patch 16)


def _oracle(K, hidden, depth, heads, ratio, grid0, seed, tiny_inputs=False):
    from transformers import Dinov2Config, Dinov2Model
    torch.manual_seed(seed)
    cfg = Dinov2Config(hidden_size=hidden, num_hidden_layers=depth, num_attention_heads=heads, mlp_ratio=ratio, image_size=16 * grid0,
                       patch_size=16, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0)
    assert cfg.layer_norm_eps == 1e-6 and not cfg.use_swiglu_ffn
    vit = Dinov2Model(cfg).eval()
    with torch.no_grad():  # make every parameter non-trivial (HF initialises biases / LayerNorm / lambda1 to 0 / 1 / 1)
        for n, p in vit.named_parameters():
            if n.endswith("lambda1"):   # away from 1 and of both signs: with lambda1 = 1 a missing scale is invisible
                p.copy_((0.2 + 1.3 * torch.rand_like(p)) * (torch.randint(0, 2, p.shape) * 2 - 1))
            elif p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        vit.embeddings.cls_token.normal_(std=0.5)
        vit.embeddings.position_embeddings.normal_(std=0.5)
        if tiny_inputs:   # the first norm1 sees tokens of variance ~1e-6: there eps = 1e-6 is half of the denominator
            vit.embeddings.cls_token.mul_(1e-3)
            vit.embeddings.position_embeddings.mul_(1e-3)
            for n, p in vit.named_parameters():
                if n.endswith(".bias"):
                    p.zero_()
    head = nn.Sequential(nn.PixelShuffle(2), nn.ConvTranspose2d(hidden // 4, K, 3, 2, 1, 1))
    with torch.no_grad():
        head[1].weight.normal_(std=0.3)
        head[1].bias.normal_(std=0.1)
    return vit.double(), head.double()


def _oracle_forward(vit, head, images):
    hs = vit(images.double(), output_hidden_states=False).last_hidden_state[:, 1:]
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
    hidden, depth, heads, ratio, grid0 = cfg
    eng = ViTEngine(K, 2, dev, hidden=hidden, depth=depth, heads=heads, mlp=ratio * hidden, patch=16, pretrain_grid=grid0, arch="dinov2", **kw)
    assert eng.ln_eps == 1e-6
    eng.load_state_dict(_state(vit, head), strict=True)
    return eng


def _compare(heat, want, grads, ref, hidden, fp32, tag):
    """the bars of tests/test_mvt_engine.py:88-118; every figure is printed before it is asserted"""
    err = (heat - want).abs()
    print(f"[{tag}] heat-maps: max abs err {err.max().item():.3e}, max err / (atol + rtol |want|) "
          f"{(err / ((1e-6 + 1e-4 * want.abs()) if fp32 else (2e-3 + (5e-2 if hidden == 128 else 1e-1) * want.abs()))).max().item():.3f}")
    if fp32:
        torch.testing.assert_close(heat, want, atol=1e-6, rtol=1e-4)
    else:
        torch.testing.assert_close(heat, want, atol=2e-3, rtol=5e-2 if hidden == 128 else 1e-1)
    assert set(grads) == set(ref)
    mask = PRE + "embeddings.mask_token"
    assert not grads[mask].any() and not ref[mask].any()      # the forward pass never reads it: exactly zero
    worst = (1.0, 0.0, "")
    seen = 0
    for k, gr in ref.items():
        got = grads[k].reshape(gr.shape)
        if gr.norm() < 1e-5:
            # analytically zero (soft-max is invariant to the key bias and to the head's per-channel bias; mask_token): only rounding noise
            assert got.norm() < (1e-5 if fp32 else 5e-3), (k, got.norm().item())
            continue
        cos = F.cosine_similarity(got.flatten(), gr.flatten(), dim=0).item()
        rel = ((got - gr).norm() / gr.norm()).item()
        if rel > worst[1]:
            worst = (cos, rel, k)
        if k.endswith(("lambda1", "cls_token", "position_embeddings")):
            seen += 1
            print(f"[{tag}] {k}: cos {cos:.6f} rel {rel:.3e}")
        if fp32:
            assert rel < 1e-4, (k, cos, rel)
        else:
            assert cos > 0.999 and rel < 0.03, (k, cos, rel)
    print(f"[{tag}] worst gradient: {worst[2]} cos {worst[0]:.6f} rel {worst[1]:.3e}")
    return seen


def check_dinov2_engine_vs_hf(dev, cfg, B, H, W, fp32, parts=None, tiny_inputs=False, tag=""):
    K = 5
    vit, head = _oracle(K, *cfg, seed=0, tiny_inputs=tiny_inputs)
    eng = _engine(dev, K, cfg, fp32, vit, head)
    gen = torch.Generator().manual_seed(1)
    images = torch.randn(B, 3, H, W, generator=gen) * (1e-3 if tiny_inputs else 1.0)
    if parts is None:
        heat, tape = eng.forward(images.to(dev), True)
    else:   # a joint pass of two batches
        assert sum(parts) == B
        heat, tape = eng.forward((images[:parts[0]].to(dev), images[parts[0]:].to(dev)), True)
    want = _oracle_forward(vit, head, images)
    assert heat.shape == want.shape == (B, K, H // 4, W // 4)
    g = torch.randn(want.shape, generator=gen)
    (want * g.double()).sum().backward()
    eng.zero_grad()
    eng.backward(tape, g.to(dev))
    grads = {k: v.detach().cpu().clone() for k, v in eng.grad_views().items()}
    ref = {PRE + k: (p.grad if p.grad is not None else torch.zeros_like(p)).float() for k, p in vit.named_parameters()}
    ref["head.upsampling_layers.1.weight"] = head[1].weight.grad.float()
    ref["head.upsampling_layers.1.bias"] = head[1].bias.grad.float()
    seen = _compare(heat.cpu(), want.detach().float(), grads, ref, cfg[0], fp32,
                    tag or f"B{B} {H}x{W} {'fp32' if fp32 else 'bf16'}{' tiny' if tiny_inputs else ''}")
    assert seen == 2 * cfg[1] + 2     # both lambda1 of every layer, cls_token and position_embeddings were compared, not skipped as zero
    return eng, images, heat


# 48 x 48: the 3 x 3 table as it is;  32 x 48: a 2 x 3 grid, the table's bicubic interpolation and its adjoint
@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,W", [(48, 48), (32, 48)])
def test_dinov2_engine_forward_backward_vs_hf(stack_backend, H, W, fp32):
    check_dinov2_engine_vs_hf(stack_backend, SMALL, 3, H, W, fp32)


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_dinov2_engine_joint_pass_of_two_batches(stack_backend, fp32):
    """labeled + unlabeled frames in one pass (2 + 1 images) against the oracle's single pass, and equal to the engine's own single pass"""
    dev = stack_backend
    eng, images, heat = check_dinov2_engine_vs_hf(dev, SMALL, 3, 32, 48, fp32, parts=(2, 1))
    assert eng.can_segment(2, 32, 48)
    single, _ = eng.forward(images.to(dev), True)
    assert torch.equal(single, heat)


def test_dinov2_layernorm_eps_matters_fp32(stack_backend):
    """inputs, [CLS] and the position table scaled by 1e-3, zero biases: the first norm1 divides by sqrt(~1e-6 + eps).  The fp32 executor holds
    the fp32 bars with Dinov2Config's 1e-6; the ViT engine's 1e-12 is off by tens of percent there"""
    dev = stack_backend
    eng, images, heat = check_dinov2_engine_vs_hf(dev, SMALL, 2, 48, 48, True, tiny_inputs=True)
    eng.ln_eps = 1e-12
    other, _ = eng.forward(images.to(dev), True)
    rel = ((other - heat).norm() / heat.norm()).item()
    print(f"heat-maps with eps 1e-12 against eps 1e-6: relative difference {rel:.3f}")
    assert rel > 0.1


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_dinov2_state_dict_names_and_strict_load_both_ways(stack_backend, fp32):
    dev = stack_backend
    vit, head = _oracle(5, *SMALL, seed=0)
    eng = _engine(dev, 5, SMALL, fp32, vit, head)
    own = eng.state_dict()
    want = {PRE + k for k in vit.state_dict()} | {"head.upsampling_layers.1.weight", "head.upsampling_layers.1.bias"}
    assert set(own) == want == set(eng.grad_views())
    sd = _state(vit, head)
    for k, v in own.items():                                                   # HF -> engine: every tensor arrived, bit for bit
        assert torch.equal(v.cpu(), sd[k].reshape(v.shape)), k
    assert own[PRE + "encoder.layer.1.layer_scale2.lambda1"].shape == (128,) and own[PRE + "embeddings.mask_token"].shape == (1, 128)
    q, kk = own[PRE + "encoder.layer.0.attention.attention.query.weight"], own[PRE + "encoder.layer.0.attention.attention.key.weight"]
    assert kk.data_ptr() - q.data_ptr() == 128 * 128 * 4                       # query / key / value are views of ONE fused GEMM weight
    from transformers import Dinov2Model
    fresh = Dinov2Model(vit.config)
    fresh.load_state_dict({k[len(PRE):]: v.cpu() for k, v in own.items() if k.startswith(PRE)}, strict=True)      # engine -> HF
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[PRE + k]), k
    with pytest.raises(KeyError):
        eng.load_state_dict({k: v for k, v in sd.items() if not k.endswith("layer_scale1.lambda1")}, strict=True)
    with pytest.raises(KeyError):
        eng.load_state_dict({**sd, PRE + "encoder.layer.0.layer_scale3.lambda1": torch.ones(128)}, strict=True)
    # a fresh engine: lambda1 = 1 (Dinov2Config.layerscale_value), mask_token = 0, all of it inside the backbone's optimiser range
    from lightning_pose_amd.vit_engine import ViTEngine
    new = ViTEngine(5, 2, dev, hidden=128, depth=2, heads=2, mlp=256, patch=16, pretrain_grid=3, arch="dinov2")
    fresh_sd = new.state_dict()
    assert torch.equal(fresh_sd[PRE + "encoder.layer.0.layer_scale1.lambda1"].cpu(), torch.ones(128))
    assert not fresh_sd[PRE + "embeddings.mask_token"].any()
    lo, hi = new.plan.group_ranges()["backbone"]
    for k, v in fresh_sd.items():
        off = (v.data_ptr() - new.P.data_ptr()) // 4
        assert (lo <= off and off + v.numel() <= hi) == k.startswith(PRE), k


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_dinov2_inference_forward_equals_training_forward(stack_backend, fp32):
    dev = stack_backend
    vit, head = _oracle(5, *SMALL, seed=0)
    eng = _engine(dev, 5, SMALL, fp32, vit, head)
    images = torch.randn(3, 3, 32, 48, generator=torch.Generator().manual_seed(2)).to(dev)
    heat, _ = eng.forward(images, True)
    assert torch.equal(eng.forward_infer(images), heat)


def test_dinov2_grad_progress_announces_only_final_tails(stack_backend):
    """the LayerScale gradients are written by the NEXT LayerNorm backward: every tail of G announced during the backward pass is final"""
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


def test_dinov2_bias_and_gelu_switches_agree(stack_backend, monkeypatch):
    """LP_VIT_BIAS_FUSED=0 / LP_VIT_GELU_FUSED=0 (the A/B switches of "vits_dino") select the LayerScale walk without column sums: the same
    gradients up to the summation order of the bias gradients"""
    dev = stack_backend
    vit, head = _oracle(5, *SMALL, seed=0)

    def grads(bias, gelu):
        monkeypatch.setenv("LP_VIT_BIAS_FUSED", bias)
        monkeypatch.setenv("LP_VIT_GELU_FUSED", gelu)
        eng = _engine(dev, 5, SMALL, False, vit, head)
        images = torch.randn(2, 3, 48, 48, generator=torch.Generator().manual_seed(5)).to(dev)
        heat, tape = eng.forward(images, True)
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


def test_dinov2_multi_view_raises(stack_backend):
    from lightning_pose_amd.vit_engine import ViTEngine
    from lightning_pose_amd.vit_engine_fp32 import Fp32ViTEngine
    for cls in (ViTEngine, Fp32ViTEngine):
        with pytest.raises(NotImplementedError, match="multi-view"):
            cls(5, 2, stack_backend, hidden=128, depth=2, heads=2, mlp=256, patch=16, pretrain_grid=3, num_views=2, arch="dinov2")
    with pytest.raises(ValueError, match="arch"):
        ViTEngine(5, 2, stack_backend, hidden=128, depth=2, heads=2, mlp=256, patch=16, pretrain_grid=3, arch="dinov3")


@pytest.mark.gpu
@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hidden,heads", [(384, 6), (768, 12)])
def test_dinov2_engine_full_width_vs_hf(hidden, heads, fp32):
    """the real widths (NP = 3 and NP = 6 of the LayerNorm walks), depth 2, on the device"""
    check_dinov2_engine_vs_hf(torch.device("cuda:0"), (hidden, 2, heads, 4, 3), 2, 32, 32, fp32)
