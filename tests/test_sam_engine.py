"""SAM mode of the ViT engine (``ViTEngine(arch="sam")`` / ``Fp32ViTEngine``) against the installed ``transformers`` ``SamVisionEncoder`` built
from a ``SamVisionConfig`` (never ``from_pretrained``), in float64 on the CPU, with the three changes of the reference's ``VisionEncoderSam``
(models/backbones/vit_sam.py: ``use_rel_pos = False`` on every layer, the neck skipped, ``pos_embed`` at the fine-tuning grid) and followed
by the PixelShuffle / ConvTranspose2d head and the soft-max.  Heat-maps and EVERY parameter gradient at the bars tests/test_dinov3_engine.py
applies to the same comparisons (fp32 executor 1e-6 + 1e-4 |want|; bf16-mixed atol 2e-3, rtol 5e-2 at hidden 128; gradients rel < 1e-4 /
cos > 0.999 and rel < 0.03).

Hidden 128, 2 heads, MLP 256, 3 layers with layer 1 global; window 3 on 80 x 80 (grid 5: four windows, three of them ragged), window 14 on
64 x 64 (grid 4: one window, 180 of its 196 rows padding), window 2 on 64 x 64 (no padding).  A control holds the cases to their purpose:
the same oracle with the pad KEYS masked - a different function - lies more than 100 x the fp32 bar away."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

transformers = pytest.importorskip("transformers")

PRE = "backbone.vision_encoder."
HEAD_KEYS = {"head.upsampling_layers.1.weight", "head.upsampling_layers.1.bias"}
SMALL = dict(hidden=128, depth=3, heads=2, mlp=256)
GLOBAL = (1,)
PRETRAIN_GRID = 8          # of the HF module's rel_pos_* on global layers (config.image_size // patch)
NECK = 32
CASES = [(3, 80), (14, 64), (2, 64)]     # (window, image side)
K = 5


def _config(window, **kw):
    from transformers import SamVisionConfig
    cfg = SamVisionConfig(hidden_size=SMALL["hidden"], num_hidden_layers=SMALL["depth"], num_attention_heads=SMALL["heads"],
                          mlp_dim=SMALL["mlp"], output_channels=NECK, patch_size=16, image_size=16 * PRETRAIN_GRID, window_size=window,
                          global_attn_indexes=list(GLOBAL), initializer_range=0.05 * (128 / SMALL["hidden"]) ** 0.5, **kw)
    # (initializer_range: the default 1e-10 would make every layer a no-op; 0.05 at width 128, and std * sqrt(width) - the gain of a Linear
    #  layer on unit-variance input - held at that value for the wider model of the device test, so that both are equally conditioned)
    assert cfg.layer_norm_eps == 1e-6 and cfg.qkv_bias and cfg.use_rel_pos and cfg.use_abs_pos and cfg.hidden_act == "gelu"
    assert cfg.attention_dropout == 0.0
    return cfg


class _Oracle(nn.Module):
    """``VisionEncoderSam`` restated around the HF module: relative positions off, ``pos_embed`` a parameter at the fine-tuning grid, its
    forward without the neck.  ``mask_pad_keys``: the control - window layers whose pad keys are masked out of the soft-max."""

    def __init__(self, window, grid, seed):
        super().__init__()
        from transformers.models.sam.modeling_sam import SamVisionEncoder
        torch.manual_seed(seed)
        self.vision_encoder = SamVisionEncoder(_config(window))
        for layer in self.vision_encoder.layers:
            layer.attn.use_rel_pos = False
        D = SMALL["hidden"]
        self.vision_encoder.pos_embed = nn.Parameter(0.5 * torch.randn(1, grid, grid, D))
        with torch.no_grad():   # every tensor non-trivial: HF leaves biases 0, LayerNorm 1 / 0, rel_pos_* 0
            for n, p in self.vision_encoder.named_parameters():
                if "rel_pos" in n or n.startswith("neck."):
                    p.normal_(std=0.3)      # (carried, never read)
                elif n.endswith("qkv.bias"):
                    p.normal_(std=0.5)      # the pad rows' q, k, v: far from zero, or padding would be nearly invisible
                elif p.dim() == 1:
                    p.add_(0.1 * torch.randn_like(p))
        self.mask_pad_keys = False

    def _masked_window_layer(self, layer, x):
        """a window layer with the pad keys masked (and only them: pad queries are cropped either way)"""
        ws = layer.window_size
        res = x
        h = layer.layer_norm1(x)
        B, gh, gw, D = h.shape
        real = torch.ones(B, gh, gw, 1, dtype=h.dtype)
        hw, pad = layer.window_partition(h, ws)
        rw, _ = layer.window_partition(real, ws)
        a = layer.attn
        nh = a.num_attention_heads
        qkv = a.qkv(hw).reshape(hw.shape[0], ws * ws, 3, nh, -1).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.reshape(3, hw.shape[0] * nh, ws * ws, -1).unbind(0)
        s = (q * a.scale) @ k.transpose(-2, -1)
        keymask = rw.reshape(hw.shape[0], 1, ws * ws).repeat_interleave(nh, 0)
        s = s.masked_fill(keymask == 0, float("-inf"))
        o = torch.softmax(s, -1) @ v
        o = o.reshape(hw.shape[0], nh, ws, ws, -1).permute(0, 2, 3, 1, 4).reshape(hw.shape[0], ws, ws, -1)
        o = layer.window_unpartition(a.proj(o), ws, pad, (gh, gw))
        x = res + o
        return x + layer.mlp(layer.layer_norm2(x))

    def forward(self, images):
        ve = self.vision_encoder
        h = ve.patch_embed.projection(images).permute(0, 2, 3, 1)      # (the wrapper's size-check bypass)
        h = h + ve.pos_embed
        for layer in ve.layers:
            if self.mask_pad_keys and layer.window_size > 0:
                h = self._masked_window_layer(layer, h)
            else:
                h = layer(h)
        return h.permute(0, 3, 1, 2)


def _oracle(window, side, seed=0):
    enc = _Oracle(window, side // 16, seed).eval()
    head = nn.Sequential(nn.PixelShuffle(2), nn.ConvTranspose2d(SMALL["hidden"] // 4, K, 3, 2, 1, 1))
    with torch.no_grad():
        head[1].weight.normal_(std=0.3)
        head[1].bias.normal_(std=0.1)
    return enc.double(), head.double()


def _oracle_forward(enc, head, images):
    logits = head(enc(images.double()))
    b, k, h, w = logits.shape
    return torch.softmax(logits.reshape(b, k, -1), -1).reshape(b, k, h, w)


def _state(enc, head):
    sd = {PRE + k: v.detach().float() for k, v in enc.vision_encoder.state_dict().items()}
    sd["head.upsampling_layers.1.weight"] = head[1].weight.detach().float()
    sd["head.upsampling_layers.1.bias"] = head[1].bias.detach().float()
    return sd


def _engine_cls(fp32):
    from lightning_pose_amd.vit_engine import ViTEngine
    from lightning_pose_amd.vit_engine_fp32 import Fp32ViTEngine
    return Fp32ViTEngine if fp32 else ViTEngine


def _engine(dev, window, side, fp32, enc=None, head=None, **kw):
    eng = _engine_cls(fp32)(K, 2, dev, patch=16, arch="sam", window=window, global_layers=GLOBAL, image_size=side, pretrain_grid=PRETRAIN_GRID,
                            neck_channels=NECK, **SMALL, **kw)
    assert eng.ln_eps == 1e-6 and eng.n_prefix == 0 and eng.plan.n_pos == (side // 16) ** 2 and eng.plan.lnf is None
    assert [L["window"] for L in eng.plan.layers] == [window, 0, window]
    if enc is not None:
        eng.load_state_dict(_state(enc, head), strict=True)
    return eng


def _carried(k):
    return "rel_pos" in k or ".neck." in k


def _grads_and_ref(eng, enc, head):
    grads = {k: v.detach().cpu().clone() for k, v in eng.grad_views().items()}
    ref = {PRE + k: (p.grad if p.grad is not None else torch.zeros_like(p)).float() for k, p in enc.vision_encoder.named_parameters()
           if not _carried(PRE + k)}
    ref["head.upsampling_layers.1.weight"] = head[1].weight.grad.float()
    ref["head.upsampling_layers.1.bias"] = head[1].bias.grad.float()
    return grads, ref


def _compare(heat, want, grads, ref, fp32, tag):
    """the bars of tests/test_dinov3_engine.py; every figure is printed before it is asserted"""
    err = (heat - want).abs()
    print(f"[{tag}] heat-maps: max abs err {err.max().item():.3e}, max err / (atol + rtol |want|) "
          f"{(err / ((1e-6 + 1e-4 * want.abs()) if fp32 else (2e-3 + 5e-2 * want.abs()))).max().item():.3f}")
    if fp32:
        torch.testing.assert_close(heat, want, atol=1e-6, rtol=1e-4)
    else:
        torch.testing.assert_close(heat, want, atol=2e-3, rtol=5e-2)
    assert set(grads) == set(ref)
    worst = (1.0, 0.0, "")
    seen = 0
    for k, gr in ref.items():
        got = grads[k].reshape(gr.shape)
        if gr.norm() < 1e-5:
            # analytically zero (the soft-max over pixels is invariant to the head's per-channel bias): only rounding noise
            assert k == "head.upsampling_layers.1.bias", k
            assert got.norm() < (1e-5 if fp32 else 5e-3), (k, got.norm().item())
            continue
        cos = F.cosine_similarity(got.flatten(), gr.flatten(), dim=0).item()
        rel = ((got - gr).norm() / gr.norm()).item()
        if rel > worst[1]:
            worst = (cos, rel, k)
        if k.endswith(("attn.qkv.bias", "pos_embed")):
            seen += 1
            print(f"[{tag}] {k}: cos {cos:.6f} rel {rel:.3e}")
        if fp32:
            assert rel < 1e-4, (k, cos, rel)
        else:
            assert cos > 0.999 and rel < 0.03, (k, cos, rel)
    print(f"[{tag}] worst gradient: {worst[2]} cos {worst[0]:.6f} rel {worst[1]:.3e}")
    return seen


def check_sam_engine_vs_hf(dev, window, side, fp32, B=3, parts=None, tag=""):
    enc, head = _oracle(window, side)
    eng = _engine(dev, window, side, fp32, enc, head)
    gen = torch.Generator().manual_seed(1)
    images = torch.randn(B, 3, side, side, generator=gen)
    if parts is None:
        heat, tape = eng.forward(images.to(dev), False)
    else:   # a joint pass of two batches
        assert sum(parts) == B
        heat, tape = eng.forward((images[:parts[0]].to(dev), images[parts[0]:].to(dev)), False)
    want = _oracle_forward(enc, head, images)
    assert heat.shape == want.shape == (B, K, side // 4, side // 4)
    g = torch.randn(want.shape, generator=gen)
    (want * g.double()).sum().backward()
    eng.zero_grad()
    eng.backward(tape, g.to(dev))
    grads, ref = _grads_and_ref(eng, enc, head)
    tag = tag or f"w{window} {side}px {'fp32' if fp32 else 'bf16'}"
    seen = _compare(heat.cpu(), want.detach().float(), grads, ref, fp32, tag)
    assert seen == SMALL["depth"] + 1          # attn.qkv.bias of every layer and pos_embed: compared, not skipped as zero
    # the window layers' qkv bias gradient on its own: the pad rows' dK / dV are part of it (their dQ is zero)
    for i in (0, 2):
        k = f"{PRE}layers.{i}.attn.qkv.bias"
        got, gr = grads[k], ref[k]
        rel = ((got - gr).norm() / gr.norm()).item()
        print(f"[{tag}] window layer {i} qkv.bias gradient: rel {rel:.3e}, |ref| {gr.norm().item():.3e}")
        assert rel < (1e-4 if fp32 else 0.03), (k, rel)
        if fp32:
            torch.testing.assert_close(got, gr, atol=1e-4 * float(gr.abs().max()), rtol=1e-4)
    return eng, images, heat


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("window,side", CASES)
def test_sam_engine_forward_backward_vs_hf(stack_backend, window, side, fp32):
    check_sam_engine_vs_hf(stack_backend, window, side, fp32)


@pytest.mark.parametrize("window,side", CASES)
def test_control_masking_the_pad_keys_is_another_function(window, side):
    """CPU only, no kernel: with the pad keys masked the oracle moves by more than 100 x the fp32 bar wherever a window is padded - so an
    engine that masked them could not pass - and not at all where nothing is padded"""
    enc, head = _oracle(window, side)
    images = torch.randn(3, 3, side, side, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = _oracle_forward(enc, head, images)
        enc.mask_pad_keys = True
        masked = _oracle_forward(enc, head, images)
    ratio = ((masked - want).abs() / (1e-6 + 1e-4 * want.abs())).max().item()
    print(f"[control w{window} {side}px] masked-pad-keys oracle: max err / fp32 bar = {ratio:.1f}")
    if (side // 16) % window:
        assert ratio > 100.0, ratio
    else:   # no padding: the masked form is the same function (and the restated window layer is the HF layer)
        assert ratio < 1e-6, ratio


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_sam_engine_joint_pass_of_two_batches(stack_backend, fp32):
    """labeled + unlabeled frames in one pass (2 + 1 images) against the oracle's single pass, and equal to the engine's own two passes"""
    dev = stack_backend
    eng, images, heat = check_sam_engine_vs_hf(dev, 3, 80, fp32, parts=(2, 1))
    assert eng.can_segment(2, 80, 80)
    a, _ = eng.forward(images[:2].to(dev), False)
    b, _ = eng.forward(images[2:].to(dev), False)
    assert torch.equal(torch.cat([a, b]), heat)


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_sam_inference_forward_equals_eval_forward(stack_backend, fp32):
    dev = stack_backend
    enc, head = _oracle(3, 80)
    eng = _engine(dev, 3, 80, fp32, enc, head)
    images = torch.randn(2, 3, 80, 80, generator=torch.Generator().manual_seed(2)).to(dev)
    heat, _ = eng.forward(images, False)
    assert torch.equal(eng.forward_infer(images), heat)


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_sam_state_dict_names_and_strict_load_both_ways(stack_backend, fp32):
    dev = stack_backend
    enc, head = _oracle(3, 80)
    eng = _engine(dev, 3, 80, fp32, enc, head)
    own = eng.state_dict()
    hf = enc.vision_encoder.state_dict()
    assert set(own) == {PRE + k for k in hf} | HEAD_KEYS
    # every HF tensor that the forward pass reads has a gradient view; rel_pos_* and neck.* are carried without one
    assert set(eng.grad_views()) == {k for k in own if not _carried(k)}
    assert sum(_carried(k) for k in own) == 2 * SMALL["depth"] + 6
    sd = _state(enc, head)
    for k, v in own.items():                                                   # HF -> engine: every tensor arrived, bit for bit
        assert v.shape == sd[k].shape and torch.equal(v.cpu(), sd[k]), k
    assert own[PRE + "pos_embed"].shape == (1, 5, 5, 128) and own[PRE + "patch_embed.projection.weight"].shape == (128, 3, 16, 16)
    assert own[PRE + "layers.0.attn.qkv.weight"].shape == (384, 128)
    assert own[PRE + "layers.0.attn.rel_pos_h"].shape == (5, 64) and own[PRE + "layers.1.attn.rel_pos_w"].shape == (2 * PRETRAIN_GRID - 1, 64)
    assert own[PRE + "neck.conv2.weight"].shape == (NECK, NECK, 3, 3)
    from transformers.models.sam.modeling_sam import SamVisionEncoder
    fresh = SamVisionEncoder(enc.vision_encoder.config)
    fresh.pos_embed = nn.Parameter(torch.zeros(1, 5, 5, 128))
    fresh.load_state_dict({k[len(PRE):]: v.cpu() for k, v in own.items() if k.startswith(PRE)}, strict=True)      # engine -> HF
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[PRE + k]), k
    with pytest.raises(KeyError):
        eng.load_state_dict({k: v for k, v in sd.items() if not k.endswith("rel_pos_h")}, strict=True)
    with pytest.raises(KeyError):
        eng.load_state_dict({**sd, PRE + "embeddings.cls_token": torch.zeros(1, 1, 128)}, strict=True)
    # a fresh engine: the trained tensors inside the backbone's optimiser range, the carried ones outside the flat buffers altogether
    new = _engine(dev, 3, 80, fp32)
    lo, hi = new.plan.group_ranges()["backbone"]
    for k, v in new.state_dict().items():
        off = (v.data_ptr() - new.P.data_ptr()) // 4
        inside = 0 <= off and off + v.numel() <= new.P.numel()
        assert inside == (not _carried(k)), k
        if inside:
            assert (lo <= off and off + v.numel() <= hi) == k.startswith(PRE), k


def test_sam_grad_progress_announces_only_final_tails(stack_backend):
    """the pad rows' share of a window layer's qkv bias gradient is in G before that layer is announced"""
    dev = stack_backend
    enc, head = _oracle(3, 80)
    eng = _engine(dev, 3, 80, False, enc, head)
    snaps = []
    eng.grad_progress = lambda off: snaps.append((off, eng.G[off:].detach().cpu().clone()))
    eng.single_backward = True
    images = torch.randn(2, 3, 80, 80, generator=torch.Generator().manual_seed(3)).to(dev)
    heat, tape = eng.forward(images, True)
    eng.zero_grad()
    eng.backward(tape, torch.randn(heat.shape, generator=torch.Generator().manual_seed(4)).to(dev))
    final = eng.G.detach().cpu().clone()
    assert len(snaps) == 1 + SMALL["depth"]
    offs = [off for off, _ in snaps]
    assert offs == sorted(offs, reverse=True) and offs[0] == eng.plan.n_backbone
    for off, snap in snaps:
        assert torch.equal(snap, final[off:]), off


@pytest.mark.parametrize("precision", ["bf16-mixed", "fp32"])
def test_sam_carried_tensors_keep_their_bits_under_fused_adam(stack_backend, precision, monkeypatch):
    """three FusedAdam steps with weight decay on the tracker's groups: rel_pos_* / neck.* are buffers, in no group, and unchanged"""
    from lightning_pose_amd import ops
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import get_model_class
    from lightning_pose_amd.models.backbones import factory as bf
    from lightning_pose_amd.optim import FusedAdam
    from lightning_pose_amd.trainer import Trainer

    dev = stack_backend
    monkeypatch.setitem(bf.SAM_CONFIGS, "vitb_sam", (128, 3, 2, 256, 16, 3, (1,), 8, 32))
    model = get_model_class("heatmap", False)(
        num_keypoints=3, loss_factory=LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None), backbone="vitb_sam", pretrained=False,
        torch_seed=0, device=dev, optimizer="AdamW", optimizer_params={"learning_rate": 1e-3}, precision=precision, image_size=80)
    eng = model.net
    carried = [k for k in eng.state_dict() if _carried(k)]
    assert len(carried) == 2 * 3 + 6
    with torch.no_grad():
        for k in carried:
            eng.state_dict()[k].normal_(std=0.3)
    before = {k: eng.state_dict()[k].detach().cpu().clone() for k in carried}
    names = {n for n, _ in model.named_parameters()}
    buffers = {n for n, _ in model.named_buffers()}
    assert not names & set(carried) and set(carried) <= buffers
    grouped = {id(p) for g in model.get_parameters() for p in g["params"]}
    assert grouped == {id(p) for p in model.parameters()}
    assert not any(model.state_dict()[k].data_ptr() in {p.data_ptr() for p in model.parameters()} for k in carried)
    gen = torch.Generator().manual_seed(0)
    kp = torch.rand(2, 3, 2, generator=gen) * 76 + 2
    batch = {"images": torch.randn(2, 3, 80, 80, generator=gen).to(dev), "keypoints": kp.reshape(2, -1).to(dev),
             "heatmaps": ops.generate_heatmaps(kp.to(dev), 80, 80, (20, 20)), "bbox": torch.tensor([[0.0, 0.0, 80.0, 80.0]] * 2).to(dev)}
    tr = Trainer(data_parallel=False)
    tr.setup(model)
    opt = model.optimizers()
    assert isinstance(opt, FusedAdam)
    for g in opt.param_groups:
        g["lr"] = 1e-3
    model.train()
    p0 = eng.P.detach().cpu().clone()
    for i in range(3):
        tr.training_batch(model, batch, i)
    assert not torch.equal(eng.P.detach().cpu(), p0)
    for k in carried:
        assert torch.equal(eng.state_dict()[k].detach().cpu(), before[k]), k


def test_sam_bias_and_gelu_switches_agree(stack_backend, monkeypatch):
    """LP_VIT_BIAS_FUSED=0 / LP_VIT_GELU_FUSED=0: the same gradients up to the summation order of the bias gradients"""
    dev = stack_backend
    enc, head = _oracle(3, 80)

    def grads(bias, gelu):
        monkeypatch.setenv("LP_VIT_BIAS_FUSED", bias)
        monkeypatch.setenv("LP_VIT_GELU_FUSED", gelu)
        eng = _engine(dev, 3, 80, False, enc, head)
        images = torch.randn(2, 3, 80, 80, generator=torch.Generator().manual_seed(5)).to(dev)
        heat, tape = eng.forward(images, False)
        eng.zero_grad()
        eng.backward(tape, (torch.randn(heat.shape, generator=torch.Generator().manual_seed(6)).to(dev)) * heat)
        return {k: v.detach().cpu().clone() for k, v in eng.grad_views().items()}

    a = grads("1", "1")
    for bias, gelu in (("0", "1"), ("1", "0")):
        b = grads(bias, gelu)
        for k in a:
            if a[k].dim() > 1 and "upsampling" not in k:
                scale = float(a[k].abs().max())
                assert scale > 0, k
                torch.testing.assert_close(a[k], b[k], atol=1e-5 * scale, rtol=0, msg=k)
        for k in a:   # the bias gradients: other summation orders, the same sums (the last fc2's, which no LayerNorm walk leaves, included)
            if k.endswith(".bias") and k.startswith(PRE):
                scale = float(a[k].abs().max())
                torch.testing.assert_close(a[k], b[k], atol=2e-2 * scale, rtol=0, msg=k)


def test_sam_refuses_what_is_out_of_scope(stack_backend):
    dev = stack_backend
    kw = dict(patch=16, **SMALL)
    for fp32 in (False, True):
        cls = _engine_cls(fp32)
        with pytest.raises(NotImplementedError, match="multi-view"):
            cls(K, 2, dev, num_views=4, arch="sam", image_size=80, **kw)
        with pytest.raises(ValueError, match="image_size"):
            cls(K, 2, dev, arch="sam", **kw)
        with pytest.raises(ValueError, match="image_size"):
            cls(K, 2, dev, arch="sam", image_size=72, **kw)
        with pytest.raises(ValueError, match="window"):
            cls(K, 2, dev, arch="sam", image_size=80, window=0, **kw)
        with pytest.raises(ValueError, match="global_layers"):
            cls(K, 2, dev, arch="sam", image_size=80, global_layers=(3,), **kw)
        with pytest.raises(ValueError, match='belong to arch="sam"'):
            cls(K, 2, dev, arch="dinov2", window=14, **kw)
        with pytest.raises(ValueError, match="registers"):
            cls(K, 2, dev, arch="sam", image_size=80, registers=4, **kw)
        eng = _engine(dev, 3, 80, fp32)
        for shape in ((1, 3, 64, 64), (1, 3, 80, 64), (1, 3, 96, 96)):     # another size, a non-square one: errors that say so
            with pytest.raises(ValueError, match=r"built for 80 x 80 images.*got " + f"{shape[2]} x {shape[3]}"):
                eng.forward(torch.zeros(shape).to(dev), False)
            with pytest.raises(ValueError, match="built for 80 x 80"):
                eng.forward_infer(torch.zeros(shape).to(dev))
    # the released configuration's defaults
    from lightning_pose_amd.vit_engine import ViTEngine
    eng = ViTEngine(K, 2, dev, hidden=128, depth=12, heads=2, mlp=256, patch=16, arch="sam", image_size=32, neck_channels=8)
    assert [L["window"] for L in eng.plan.layers] == [14, 14, 0, 14, 14, 0, 14, 14, 0, 14, 14, 0]
    sd = eng.state_dict()
    assert sd[PRE + "layers.0.attn.rel_pos_h"].shape == (27, 64) and sd[PRE + "layers.2.attn.rel_pos_h"].shape == (127, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_sam_engine_full_width_vs_hf(fp32, monkeypatch):
    """ViT-B's width (12 heads, NP = 6 of the LayerNorm walks, 4608-byte qkv rows), depth 3, window 14 on a 16 x 16 grid (four windows of
    196 tokens, all ragged), on the device"""
    monkeypatch.setitem(SMALL, "hidden", 768)
    monkeypatch.setitem(SMALL, "heads", 12)
    monkeypatch.setitem(SMALL, "mlp", 3072)
    dev = torch.device("cuda:0")
    enc, head = _oracle(14, 256)
    eng = _engine(dev, 14, 256, fp32, enc, head)
    images = torch.randn(1, 3, 256, 256, generator=torch.Generator().manual_seed(1))
    heat, tape = eng.forward(images.to(dev), False)
    want = _oracle_forward(enc, head, images).detach().float()
    err = (heat.cpu() - want).abs()
    print(f"[full width {'fp32' if fp32 else 'bf16'}] heat-maps: max abs err {err.max().item():.3e}")
    # (hidden 768: the bf16 bar of tests/test_dinov3_engine.py at the wider widths, rtol 1e-1)
    torch.testing.assert_close(heat.cpu(), want, atol=1e-6 if fp32 else 2e-3, rtol=1e-4 if fp32 else 1e-1)
