"""Torch-tensor front end of the lp_hip C ABI: device checks, stream plumbing, autograd glue.

Every function here enqueues hand-written HIP kernels from ``liblp_hip.so`` on torch's current stream.  PyTorch is
used for device memory, streams and autograd bookkeeping only.  There is no CPU path: tensors must live on a ROCm
device, otherwise ``LpHipUnavailable`` is raised.
"""

from __future__ import annotations

import ctypes as C
import os
import functools
from typing import Sequence

import numpy as np
import torch

from . import _lib, _tables
from ._lib import LpHipUnavailable, check

__all__ = [
    "decode", "DecodeFrameMap", "generate_heatmaps", "heatmap_mse", "unimodal_mse", "temporal_loss", "pca_loss",
    "rmse", "keypoint_metrics", "PcaMetricSpec", "require_device", "frames_resize", "frames_augment", "labeled_keypoints", "bbox_from_keypoints", "bbox_smooth", "frames_crop_resize", "patch_mask", "mv3d_plan", "mv3d_fill", "mv3d_finish",
]


def require_device(*tensors: torch.Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise LpHipUnavailable(
                "lightning_pose_amd ops run only on a ROCm device (got a CPU tensor); there is no CPU fallback")
        if t.device.index is not None and t.device.index != torch.cuda.current_device():
            raise LpHipUnavailable(f"tensor on {t.device} but the current device is cuda:{torch.cuda.current_device()}: kernels launch on the "
                                   "current device's stream - call torch.cuda.set_device (one process per GPU)")
        dev = t.device
    return dev


def require_device_type(device: torch.device) -> None:
    if device.type != "cuda":
        raise LpHipUnavailable(f"lightning_pose_amd needs a ROCm device (got {device}); there is no CPU fallback")
    if device.index is not None and device.index != torch.cuda.current_device():
        torch.cuda.set_device(device)  # the engine's device becomes the process's current device (one process per GPU)


def _stream() -> C.c_void_p:
    """torch's current stream on the CURRENT device.  Kernels are launched on the current device, so a model's device must be the
    current one: Engine / ViTEngine make it so when they are built (one process per GPU, as the reference's DDP), and require_device
    refuses tensors of another device instead of launching device-0 kernels on device-1 pointers."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: torch.Tensor | None) -> C.c_void_p | None:
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


# --------------------------------------------------------------------------------------------------------
# decode
# --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=16)
def _device_tables(h: int, w: int, ds: int, dev: torch.device):
    ty, tx = _tables.axis_tables(h, ds), _tables.axis_tables(w, ds)
    keep = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
            (ty["row_base"], ty["row_taps"], tx["col_start"], tx["col_taps"], tx["colT_start"], tx["colT_taps"])]
    struct = _lib.DecodeTables(*[t.data_ptr() for t in keep], ty["ty"], tx["tx"], tx["tc"])
    return struct, keep


class DecodeFrameMap:
    """undo-affine + model->frame epilogue parameters (reference: data/utils.py:191-234, data/bboxes.py:222-288)."""

    def __init__(self, transforms: torch.Tensor | None, is_multiview: bool, bbox: torch.Tensor | None, num_views: int,
                 model_h: int, model_w: int, num_keypoints: int):
        self.keep = []
        self.rows_needed: int | None = None
        self.bbox_rows: int | None = None
        self._tf = self._bbox = None
        tf_mode, tf = _lib.TF_NONE, None
        if transforms is not None and transforms.shape[-1] == 3:
            tf = _f32c(transforms)
            if is_multiview:
                tf_mode = _lib.TF_PER_VIEW
            elif tf.dim() == 2 or tf.shape[0] == 1:
                # one matrix for the whole batch: (2, 3), or (1, 2, 3) as the DALI pipeline hands it over - the reference replicates a
                # single inverse over the batch (data/utils.py:176-180)
                tf_mode = _lib.TF_SINGLE
            else:
                tf_mode = _lib.TF_PER_FRAME
                self.rows_needed = int(tf.shape[0])   # one matrix per frame: checked against the batch where it is known (check_batch)
            self._tf = tf
            self.keep.append(tf)
        bb = None
        if bbox is not None:
            bb = _f32c(bbox)
            self.bbox_rows = int(bb.shape[0]) if bb.dim() == 2 else None
            self._bbox = bb
            self.keep.append(bb)
        self.struct = _lib.FrameMap(_p(tf), tf_mode, _p(bb), 4 * num_views, max(1, num_keypoints // num_views),
                                    float(model_h), float(model_w))

    def check_batch(self, b: int, device: torch.device | None = None) -> None:
        """Called where the batch (and its device) is known.  The kernels index the per-frame tables by frame: a table shorter than the batch
        would be read out of bounds (the reference fails in torch.bmm / broadcasting on the same inputs); and they dereference raw pointers:
        tables the caller left on another device (the reference moves its inverse matrices to the keypoints' device, data/utils.py:170-172)
        are moved here."""
        if self.rows_needed is not None and self.rows_needed != b:
            raise ValueError(f"{self.rows_needed} affine transforms for a batch of {b} frames (one per frame, or a single (2, 3) / (1, 2, 3))")
        if self.bbox_rows is not None and self.bbox_rows != b:
            if self.bbox_rows != 1:
                raise ValueError(f"{self.bbox_rows} bounding boxes for a batch of {b} frames")
            self._bbox = self._bbox.expand(b, -1).contiguous()   # one box for every frame: what broadcasting gives the reference (data/bboxes.py:222-288)
            self.keep.append(self._bbox)
            self.struct.bbox = self._bbox.data_ptr()
            self.bbox_rows = b
        if device is not None:
            if self._tf is not None and self._tf.device != device:
                self._tf = self._tf.to(device)
                self.keep.append(self._tf)
                self.struct.transforms = self._tf.data_ptr()
            if self._bbox is not None and self._bbox.device != device:
                self._bbox = self._bbox.to(device)
                self.keep.append(self._bbox)
                self.struct.bbox = self._bbox.data_ptr()


def _prune_env() -> str:
    """LP_DECODE_PRUNE: "auto" (default / unset / empty), "0" or "1" - anything else is a configuration error, not a silent default"""
    v = os.environ.get("LP_DECODE_PRUNE", "").strip().lower()
    if v in ("", "auto"):
        return "auto"
    if v in ("0", "1"):
        return v
    raise ValueError(f"LP_DECODE_PRUNE must be auto, 0 or 1 (got {v!r})")


class _DecodePruneAuto:
    """Chooses between the plain and the exactly-pruned decode kernels (the `prune` argument of lp_decode_fwd / lp_decode_bwd) from what the
    decode itself reports.

    stats[..., 1] of lp_decode_fwd is sum exp(T (y - max y)) over the up-sampled map = the number of pixels that carry weight in the
    soft-argmax: ~2 - 10 on the peaked maps of a trained head (T = 1000), ~all 147 456 on the flat maps of an untrained one.  Pruning pays
    (forward 1.4x, backward 1.8x, profiles/archive/r02k_decode_microbench.jsonl) when most maps are peaked and costs when they are flat, and which
    regime a run is in changes once, early in training.  So every PERIOD-th call (and the FIRST-th) the fraction of peaked maps is reduced
    on the device and copied to pinned host memory WITHOUT a synchronisation; a later call picks the value up once its event has
    completed and flips the choice if needed.  LP_DECODE_PRUNE=0 / 1 pins the choice instead (read per call, here on the host: the
    library itself holds no switch since round 5).

    One instance per OWNER (a tracker: HeatmapTracker._decode passes its own; stand-alone ops.decode calls share `_decode_prune_default`),
    so one model's maps never steer another's kernels and a fresh model starts from the plain kernels.  While the current stream is being
    captured into a HIP graph nothing here runs - no event query, no pinned allocation, no copy, no counter: a replayed graph keeps the
    kernels it was captured with, and the eager steps around captures are where the choice is re-evaluated."""

    PERIOD, FIRST, PEAKED_FRACTION_OF_PIXELS, PEAKED_MAPS = 32, 2, 0.01, 0.5

    def __init__(self) -> None:
        self.calls, self.pending, self.want = 0, None, 0   # want: this owner's current choice (0 plain, 1 pruned)
        self.last = -2                                      # what the most recent decode call was given (-2: none yet)

    @property
    def state(self) -> int:
        """the `prune` argument of this owner's most recent decode call (tests, bench): 0 plain, 1 pruned, -2 no call yet"""
        return self.last

    @staticmethod
    def _capturing() -> bool:
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    def before(self) -> int:
        """the `prune` argument for the call about to be made"""
        env = _prune_env()
        if env != "auto":          # pinned by the environment
            self.pending = None
            self.last = int(env)
            return self.last
        if not self._capturing() and self.pending is not None:
            host, ev = self.pending
            if ev is None or ev.query():
                self.want = 1 if float(host[0]) >= self.PEAKED_MAPS else 0
                self.pending = None
        self.last = self.want
        return self.last

    def after(self, stats: torch.Tensor, n_up: int) -> None:
        if _prune_env() != "auto" or self._capturing():
            return
        self.calls += 1
        if self.pending is not None or not (self.calls == self.FIRST or self.calls % self.PERIOD == 0):
            return
        frac = (stats[..., 1] < self.PEAKED_FRACTION_OF_PIXELS * n_up).float().mean().reshape(1)
        if stats.device.type == "cuda":
            host = torch.empty(1, dtype=torch.float32, pin_memory=True)
            host.copy_(frac, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.pending = (host, ev)
        else:
            self.pending = (frac.detach().clone(), None)


_decode_prune_default = _DecodePruneAuto()
_decode_prune_auto = _decode_prune_default   # (the name round 3's tests and bench read)


class _DecodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heat, ds, temperature, frame_map, prune):
        require_device(heat)
        ctx.in_dtype = heat.dtype
        heat = heat.to(torch.float32).contiguous()
        b, k, h, w = heat.shape
        frame_map.check_batch(b, heat.device)
        tables, keep = _device_tables(h, w, ds, heat.device)
        kp_aug = torch.empty(b, k, 2, device=heat.device, dtype=torch.float32)
        kp_frame = torch.empty_like(kp_aug)
        conf = torch.empty(b, k, device=heat.device, dtype=torch.float32)
        stats = torch.empty(b, k, 4, device=heat.device, dtype=torch.float32)
        mode = prune.before()
        check(_lib.lib().lp_decode_fwd(_p(heat), b, k, h, w, ds, float(temperature), C.byref(tables),
                                       C.byref(frame_map.struct), _p(kp_aug), _p(kp_frame), _p(conf), _p(stats), mode, _stream()),
              "lp_decode_fwd")
        prune.after(stats, h * w * (4 ** int(ds)))
        ctx.save_for_backward(heat, stats)
        ctx.args = (ds, float(temperature), frame_map, tables, keep, mode)
        ctx.mark_non_differentiable(conf)
        return kp_aug.reshape(b, 2 * k), kp_frame.reshape(b, 2 * k), conf

    @staticmethod
    def backward(ctx, g_aug, g_frame, _g_conf):
        heat, stats = ctx.saved_tensors
        ds, temperature, frame_map, tables, _keep, mode = ctx.args   # (the backward runs the kernel family its forward ran)
        b, k, h, w = heat.shape
        ga = _f32c(g_aug) if g_aug is not None else None
        gf = _f32c(g_frame) if g_frame is not None else None
        g_heat = torch.empty_like(heat)
        check(_lib.lib().lp_decode_bwd(_p(heat), b, k, h, w, ds, temperature, C.byref(tables), C.byref(frame_map.struct),
                                       _p(stats), _p(ga), _p(gf), _p(g_heat), 0, mode, _stream()), "lp_decode_bwd")
        return g_heat.to(ctx.in_dtype), None, None, None, None


class _FrameMapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kp, frame_map):
        require_device(kp)
        x = _f32c(kp)
        b, k = x.shape[0], x.shape[1] // 2
        frame_map.check_batch(b, x.device)
        out = torch.empty_like(x)
        check(_lib.lib().lp_frame_map_apply(_p(x), b, k, C.byref(frame_map.struct), 0, _p(out), _stream()), "lp_frame_map_apply")
        ctx.frame_map = frame_map
        return out

    @staticmethod
    def backward(ctx, g):
        g = _f32c(g)
        b, k = g.shape[0], g.shape[1] // 2
        out = torch.empty_like(g)
        check(_lib.lib().lp_frame_map_apply(_p(g), b, k, C.byref(ctx.frame_map.struct), 1, _p(out), _stream()), "lp_frame_map_apply")
        return out, None


def frame_map_apply(keypoints: torch.Tensor, frame_map: DecodeFrameMap) -> torch.Tensor:
    """keypoints (B, 2K) in model px -> frame px through the undo-affine / bbox map (differentiable)."""
    return _FrameMapFn.apply(keypoints, frame_map)


def decode(heatmaps: torch.Tensor, downsample_factor: int, temperature: float, frame_map: DecodeFrameMap,
           prune: "_DecodePruneAuto | None" = None):
    """heatmaps (B,K,h,w) -> keypoints in model px (B,2K), keypoints in frame px (B,2K), confidences (B,K).
    ``prune``: the caller's own plain / pruned-kernel chooser (a tracker passes its own, see _DecodePruneAuto); default: a shared one."""
    return _DecodeFn.apply(heatmaps, int(downsample_factor), float(temperature), frame_map, prune or _decode_prune_default)


# --------------------------------------------------------------------------------------------------------
# heat-map targets / losses
# --------------------------------------------------------------------------------------------------------

class _HeatmapGenFn(torch.autograd.Function):
    """generate_heatmaps with the keypoints attached (keep_gradients=True): lp_heatmap_gen forward, lp_heatmap_gen_bwd backward"""

    @staticmethod
    def forward(ctx, keypoints, height, width, output_shape, sigma, visibility):
        out = generate_heatmaps(keypoints.detach(), height, width, output_shape, sigma, visibility)
        ctx.save_for_backward(_f32c(keypoints))
        ctx.args = (int(height), int(width), tuple(output_shape), float(sigma),
                    None if visibility is None else visibility.to(device=keypoints.device, dtype=torch.int32).contiguous())
        ctx.in_dtype = keypoints.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        (kp,) = ctx.saved_tensors
        height, width, (h, w), sigma, vis = ctx.args
        b, k, _ = kp.shape
        gkp = torch.empty_like(kp)
        check(_lib.lib().lp_heatmap_gen_bwd(_p(kp), _p(vis), b, k, height, width, h, w, sigma, _p(_f32c(g)), _p(gkp), _stream()),
              "lp_heatmap_gen_bwd")
        return gkp.to(ctx.in_dtype), None, None, None, None, None


def generate_heatmaps_with_grad(keypoints: torch.Tensor, height: int, width: int, output_shape: tuple[int, int], sigma: float = 1.25,
                                visibility: torch.Tensor | None = None) -> torch.Tensor:
    return _HeatmapGenFn.apply(keypoints, height, width, tuple(output_shape), sigma, visibility)


def generate_heatmaps(keypoints: torch.Tensor, height: int, width: int, output_shape: tuple[int, int], sigma: float = 1.25,
                      visibility: torch.Tensor | None = None) -> torch.Tensor:
    require_device(keypoints)
    kp = _f32c(keypoints)
    if kp.dim() != 3 or kp.shape[2] != 2:
        raise ValueError(f"keypoints must be (B, K, 2), got {tuple(kp.shape)}")
    b, k, _ = kp.shape
    h, w = output_shape
    vis = None
    if visibility is not None:
        if tuple(visibility.shape) != (b, k):
            raise ValueError(f"visibility must be {(b, k)}, got {tuple(visibility.shape)}")
        vis = visibility.to(device=kp.device, dtype=torch.int32).contiguous()
    out = torch.empty(b, k, h, w, device=kp.device, dtype=torch.float32)
    check(_lib.lib().lp_heatmap_gen(_p(kp), _p(vis), b, k, int(height), int(width), h, w, float(sigma), _p(out), _stream()),
          "lp_heatmap_gen")
    return out


def heatmap_confidence(heatmaps: torch.Tensor, locs: torch.Tensor, radius: int) -> torch.Tensor:
    require_device(heatmaps, locs)
    heat, lc = _f32c(heatmaps), _f32c(locs)
    b, k, h, w = heat.shape
    if lc.shape != (b, k, 2):
        raise ValueError(f"locs must be {(b, k, 2)}, got {tuple(lc.shape)}")
    out = torch.empty(b, k, device=heat.device, dtype=torch.float32)
    check(_lib.lib().lp_heatmap_confidence(_p(heat), _p(lc), b, k, h, w, int(radius), _p(out), _stream()), "lp_heatmap_confidence")
    return out


class _HeatmapLossFn(torch.autograd.Function):
    """masked mean over the labelled maps of a per-map sum: kind = HM_MSE / HM_KL / HM_JS"""

    @staticmethod
    def forward(ctx, targ, pred, kind):
        require_device(targ, pred)
        ctx.in_dtype = pred.dtype
        targ, pred = _f32c(targ), _f32c(pred)
        if pred.dim() != 4 or targ.shape != pred.shape:   # raw pointers from here on: a shape the reference's mse_loss would refuse
            raise ValueError(f"heat-map targets {tuple(targ.shape)} and predictions {tuple(pred.shape)} must both be (B, K, h, w)")
        b, k, h, w = pred.shape
        ws = torch.empty(_lib.lib().lp_heatmap_mse_workspace_bytes(b, k), device=pred.device, dtype=torch.uint8)
        loss = torch.empty(1, device=pred.device, dtype=torch.float32)
        check(_lib.lib().lp_heatmap_loss_fwd(kind, _p(targ), _p(pred), b, k, h, w, _p(loss), _p(ws), _stream()), "lp_heatmap_loss_fwd")
        ctx.save_for_backward(targ, pred, ws)
        ctx.kind = kind
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        targ, pred, ws = ctx.saved_tensors
        b, k, h, w = pred.shape
        g = torch.empty_like(pred)
        go = _f32c(gout).reshape(1)
        check(_lib.lib().lp_heatmap_loss_bwd(ctx.kind, _p(targ), _p(pred), b, k, h, w, _p(ws), _p(go), _p(g), 0, _stream()),
              "lp_heatmap_loss_bwd")
        return None, g.to(ctx.in_dtype), None


def heatmap_mse(targets: torch.Tensor, predictions: torch.Tensor) -> torch.Tensor:
    return _HeatmapLossFn.apply(targets, predictions, _lib.HM_MSE)


def heatmap_kl(targets: torch.Tensor, predictions: torch.Tensor) -> torch.Tensor:
    return _HeatmapLossFn.apply(targets, predictions, _lib.HM_KL)


def heatmap_js(targets: torch.Tensor, predictions: torch.Tensor) -> torch.Tensor:
    return _HeatmapLossFn.apply(targets, predictions, _lib.HM_JS)


class _UnimodalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kp_aug, pred, conf, img_h, img_w, sigma, thr):
        require_device(kp_aug, pred, conf)
        ctx.in_dtype = pred.dtype
        kp, pred, conf = _f32c(kp_aug), _f32c(pred), _f32c(conf)
        s, k, h, w = pred.shape
        if kp.numel() != s * k * 2 or tuple(conf.shape) != (s, k):
            raise ValueError(f"unimodal_mse: keypoints {tuple(kp.shape)} / confidences {tuple(conf.shape)} do not match heat-maps {tuple(pred.shape)}")
        ws = torch.empty(_lib.lib().lp_heatmap_mse_workspace_bytes(s, k), device=pred.device, dtype=torch.uint8)
        loss = torch.empty(1, device=pred.device, dtype=torch.float32)
        check(_lib.lib().lp_unimodal_mse_fwd(_p(kp), _p(pred), _p(conf), s, k, img_h, img_w, h, w, sigma, thr, _p(loss), _p(ws),
                                             _stream()), "lp_unimodal_mse_fwd")
        ctx.save_for_backward(kp, pred, ws)
        ctx.args = (img_h, img_w, sigma)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        kp, pred, ws = ctx.saved_tensors
        img_h, img_w, sigma = ctx.args
        s, k, h, w = pred.shape
        g = torch.empty_like(pred)
        go = _f32c(gout).reshape(1)
        check(_lib.lib().lp_unimodal_mse_bwd(_p(kp), _p(pred), s, k, img_h, img_w, h, w, sigma, _p(ws), _p(go), _p(g), 0,
                                             _stream()), "lp_unimodal_mse_bwd")
        return None, g.to(ctx.in_dtype), None, None, None, None, None


def unimodal_mse(keypoints_pred_augmented: torch.Tensor, heatmaps_pred: torch.Tensor, confidences: torch.Tensor,
                 image_height: int, image_width: int, sigma: float = 1.25, prob_threshold: float = 0.0) -> torch.Tensor:
    return _UnimodalFn.apply(keypoints_pred_augmented, heatmaps_pred, confidences, int(image_height), int(image_width),
                             float(sigma), float(prob_threshold))


# --------------------------------------------------------------------------------------------------------
# keypoint-space losses
# --------------------------------------------------------------------------------------------------------

class _UnitGradFn(torch.autograd.Function):
    """loss whose gradient for unit upstream was produced together with the value (one launch)."""

    @staticmethod
    def forward(ctx, kp, loss, grad_unit):
        ctx.save_for_backward(grad_unit)
        ctx.shape = kp.shape
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grad_unit,) = ctx.saved_tensors
        return (grad_unit * gout).reshape(ctx.shape), None, None


_EPS_CACHE: dict = {}


def _device_epsilon(epsilon: torch.Tensor, k: int, dev: torch.device) -> torch.Tensor:
    """per-keypoint epsilon vector on the device; uploaded once per (tensor, k, device) - a host-to-device copy every step would
    serialise the host with the launch queue and cannot be captured into a HIP graph"""
    key = (id(epsilon), k, str(dev))
    hit = _EPS_CACHE.get(key)
    if hit is not None and hit[0] is epsilon and hit[1] == epsilon._version:
        return hit[2]
    eps = epsilon.to(device=dev, dtype=torch.float32).reshape(-1)
    eps = eps.expand(k).contiguous() if eps.numel() == 1 else eps.contiguous()
    if eps.numel() != k:
        raise ValueError(f"temporal epsilon must be a scalar or have one entry per keypoint ({k}), got {eps.numel()}")
    if len(_EPS_CACHE) > 64:
        _EPS_CACHE.clear()
    _EPS_CACHE[key] = (epsilon, epsilon._version, eps)
    return eps


def temporal_loss(keypoints: torch.Tensor, confidences: torch.Tensor | None, epsilon: torch.Tensor, prob_threshold: float):
    """keypoints (S, 2K) -> scalar (reference losses/losses.py:674-703)."""
    require_device(keypoints)
    kp = _f32c(keypoints)
    s = kp.shape[0]
    k = kp.shape[1] // 2
    conf = _f32c(confidences) if confidences is not None else None
    if kp.dim() != 2 or kp.shape[1] % 2 or (conf is not None and tuple(conf.shape) != (s, k)):
        raise ValueError(f"temporal loss: keypoints {tuple(kp.shape)} must be (S, 2K) and confidences (S, K)")
    eps = _device_epsilon(epsilon, k, kp.device)
    loss = torch.empty(1, device=kp.device, dtype=torch.float32)
    grad = torch.empty_like(kp)
    check(_lib.lib().lp_temporal_fwd_bwd(_p(kp), _p(conf), s, k, _p(eps), float(prob_threshold), _p(loss), _p(grad), _stream()),
          "lp_temporal_fwd_bwd")
    return _UnitGradFn.apply(keypoints, loss.reshape(()), grad)


class _TemporalHeatmapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, conf, eps, thr, kind):
        require_device(pred, conf)
        ctx.in_dtype = pred.dtype
        pred, conf = _f32c(pred), _f32c(conf)
        s, k, h, w = pred.shape
        ws = torch.empty(_lib.lib().lp_temporal_heatmap_workspace_bytes(s, k), device=pred.device, dtype=torch.uint8)
        loss = torch.empty(1, device=pred.device, dtype=torch.float32)
        check(_lib.lib().lp_temporal_heatmap_fwd(kind, _p(pred), _p(conf), s, k, h, w, _p(eps), float(thr), _p(loss), _p(ws), _stream()),
              "lp_temporal_heatmap_fwd")
        ctx.save_for_backward(pred, ws)
        ctx.kind = kind
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        pred, ws = ctx.saved_tensors
        s, k, h, w = pred.shape
        g = torch.empty_like(pred)
        go = _f32c(gout).reshape(1)
        check(_lib.lib().lp_temporal_heatmap_bwd(ctx.kind, _p(pred), s, k, h, w, _p(ws), _p(go), _p(g), 0, _stream()),
              "lp_temporal_heatmap_bwd")
        return g.to(ctx.in_dtype), None, None, None, None


def temporal_heatmap_distances(heatmaps_pred: torch.Tensor, kind: int) -> torch.Tensor:
    """(S, K, h, w) -> (S-1, K) distances between consecutive heat-maps (TemporalHeatmapLoss.compute_loss, reference :793-829);
    no autograd (the differentiable form is ``temporal_heatmap_loss``)."""
    require_device(heatmaps_pred)
    pred = _f32c(heatmaps_pred)
    s, k, h, w = pred.shape
    if s < 2:
        return torch.zeros(0, k, device=pred.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().lp_temporal_heatmap_workspace_bytes(s, k), device=pred.device, dtype=torch.uint8)
    conf = torch.ones(s, k, device=pred.device, dtype=torch.float32)
    eps = torch.zeros(k, device=pred.device, dtype=torch.float32)
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    check(_lib.lib().lp_temporal_heatmap_fwd(kind, _p(pred), _p(conf), s, k, h, w, _p(eps), 0.0, _p(loss), _p(ws), _stream()),
          "lp_temporal_heatmap_fwd")
    return ws[: (s - 1) * k * 4].view(torch.float32).reshape(s - 1, k).clone()


def temporal_heatmap_loss(heatmaps_pred: torch.Tensor, confidences: torch.Tensor, epsilon: torch.Tensor, prob_threshold: float,
                          kind: int) -> torch.Tensor:
    """(S, K, h, w) heat-maps, (S, K) confidences -> scalar (reference losses/losses.py:841-869); kind = HM_MSE | HM_KL."""
    k = heatmaps_pred.shape[1]
    eps = _device_epsilon(epsilon, k, heatmaps_pred.device)
    if tuple(confidences.shape) != tuple(heatmaps_pred.shape[:2]):
        raise ValueError(f"confidences must be {tuple(heatmaps_pred.shape[:2])}, got {tuple(confidences.shape)}")
    return _TemporalHeatmapFn.apply(heatmaps_pred, confidences, eps, float(prob_threshold), kind)


def pca_loss(keypoints: torch.Tensor, index: torch.Tensor, mean: torch.Tensor, kept_eigenvectors: torch.Tensor, epsilon: float):
    """keypoints (S, 2K); index (rows, points) int32 keypoint ids per PCA sample -> scalar (losses/losses.py:548-573)."""
    require_device(keypoints, index, mean, kept_eigenvectors)
    kp = _f32c(keypoints)
    # raw pointers go to the kernel: every operand must be dense row-major fp32 / int32 (a transposed view of the eigenvector matrix,
    # for instance, keeps its strides through .to(device))
    mean, kept_eigenvectors = _f32c(mean), _f32c(kept_eigenvectors)
    index = index.to(torch.int32).contiguous()
    s, k = kp.shape[0], kp.shape[1] // 2
    rows, pts = index.shape
    if mean.numel() != 2 * pts or kept_eigenvectors.dim() != 2 or kept_eigenvectors.shape[1] != 2 * pts:
        raise ValueError(f"pca loss: mean {tuple(mean.shape)} / eigenvectors {tuple(kept_eigenvectors.shape)} do not span the "
                         f"{2 * pts} coordinates of a sample ({pts} points)")
    loss = torch.empty(1, device=kp.device, dtype=torch.float32)
    grad = torch.empty_like(kp)
    check(_lib.lib().lp_pca_fwd_bwd(_p(kp), s, k, _p(index), rows, pts, _p(mean), _p(kept_eigenvectors),
                                    kept_eigenvectors.shape[0], float(epsilon), _p(loss), _p(grad), _stream()), "lp_pca_fwd_bwd")
    return _UnitGradFn.apply(keypoints, loss.reshape(()), grad)


class PcaMetricSpec:
    """One PCA table of ``keypoint_metrics``: the index table (rows, points) of ``KeypointPCA.index_table`` with the fitted mean and kept
    eigenvectors on ``device``.  The index table is kept twice: on the device for the kernel, on the host for the check before the launch."""

    def __init__(self, index, mean: torch.Tensor, kept_eigenvectors: torch.Tensor, device: torch.device | str) -> None:
        index_host = np.ascontiguousarray(index.detach().cpu().numpy() if torch.is_tensor(index) else np.asarray(index)).astype(np.int32)
        if index_host.ndim != 2 or index_host.size == 0:
            raise ValueError(f"index must be a non-empty (rows, points) table, got shape {index_host.shape}")
        self.index_host = index_host
        self.rows, self.points = (int(n) for n in index_host.shape)
        dev = torch.device(device)
        self.index = torch.from_numpy(index_host).to(dev)
        # raw pointers go to the kernel: dense row-major fp32 (as pca_loss)
        self.mean = _f32c(torch.as_tensor(mean)).reshape(-1).to(dev)
        self.kept_eigenvectors = _f32c(torch.as_tensor(kept_eigenvectors)).to(dev)
        if self.mean.numel() != 2 * self.points or self.kept_eigenvectors.dim() != 2 or self.kept_eigenvectors.shape[1] != 2 * self.points:
            raise ValueError(f"pca metric: mean {tuple(self.mean.shape)} / eigenvectors {tuple(self.kept_eigenvectors.shape)} do not span the "
                             f"{2 * self.points} coordinates of a sample ({self.points} points)")
        self.ncomp = int(self.kept_eigenvectors.shape[0])

    @classmethod
    def from_pca(cls, pca, num_keypoints: int, device: torch.device | str) -> "PcaMetricSpec":
        """from a fitted ``utils.pca.KeypointPCA``"""
        return cls(pca.index_table(num_keypoints), pca.parameters["mean"], pca.parameters["kept_eigenvectors"], device)

    def struct(self) -> _lib.PcaSpec:
        return _lib.PcaSpec(self.index.data_ptr(), self.index_host.ctypes.data, self.rows, self.points, self.mean.data_ptr(),
                            self.kept_eigenvectors.data_ptr() if self.ncomp else None, self.ncomp)


def keypoint_metrics(keypoints_pred: torch.Tensor, keypoints_true: torch.Tensor | None = None, pca_singleview: PcaMetricSpec | None = None,
                     pca_multiview: PcaMetricSpec | None = None, *, temporal: bool = True) -> dict[str, torch.Tensor]:
    """(T, K, 2) or (T, 2K) device predictions -> the requested (T, K) fp32 metric tables, on the device, from ONE launch of
    ``lp_kp_metrics`` (reference metrics.py:47-184): ``"temporal_norm"`` (``temporal``), ``"pixel_error"`` (``keypoints_true`` given, same
    shape), ``"pca_singleview_error"`` / ``"pca_multiview_error"`` (their spec given).  Nothing is read back."""
    require_device(keypoints_pred, keypoints_true)
    if keypoints_pred.dim() not in (2, 3) or (keypoints_pred.dim() == 3 and keypoints_pred.shape[-1] != 2) or keypoints_pred.shape[-1] % 2 \
            or keypoints_pred.numel() == 0:
        raise ValueError(f"keypoints_pred must be a non-empty (T, K, 2) or (T, 2K), got {tuple(keypoints_pred.shape)}")
    pred = _f32c(keypoints_pred)
    t, k = int(pred.shape[0]), int(pred.numel() // (2 * pred.shape[0]))
    true = None
    if keypoints_true is not None:
        true = _f32c(keypoints_true)
        if true.numel() != pred.numel() or true.shape[0] != t:
            raise ValueError(f"keypoints_true {tuple(keypoints_true.shape)} and keypoints_pred {tuple(keypoints_pred.shape)} differ in size")
    names = [n for n, wanted in (("pixel_error", true is not None), ("temporal_norm", temporal), ("pca_singleview_error", pca_singleview is not None),
                                 ("pca_multiview_error", pca_multiview is not None)) if wanted]
    if not names:
        raise ValueError("keypoint_metrics: nothing to compute (no labels, temporal=False, no PCA spec)")
    for spec in (pca_singleview, pca_multiview):
        if spec is not None:
            require_device(spec.index, spec.mean, spec.kept_eigenvectors)
    out = {n: torch.empty(t, k, device=pred.device, dtype=torch.float32) for n in names}
    sv = None if pca_singleview is None else pca_singleview.struct()
    mv = None if pca_multiview is None else pca_multiview.struct()
    check(_lib.lib().lp_kp_metrics(_p(pred), _p(true), t, k, None if sv is None else C.byref(sv), None if mv is None else C.byref(mv),
                                   _p(out.get("pixel_error")), _p(out.get("temporal_norm")), _p(out.get("pca_singleview_error")),
                                   _p(out.get("pca_multiview_error")), _stream()), "lp_kp_metrics")
    return out


def rmse(keypoints_targ: torch.Tensor, keypoints_pred: torch.Tensor) -> torch.Tensor:
    require_device(keypoints_targ, keypoints_pred)
    t, p = _f32c(keypoints_targ), _f32c(keypoints_pred)
    if t.shape != p.shape or t.numel() % 2:
        raise ValueError(f"rmse: target {tuple(t.shape)} and predicted {tuple(p.shape)} keypoints must both be (B, 2K)")
    loss = torch.empty(1, device=p.device, dtype=torch.float32)
    check(_lib.lib().lp_rmse_fwd(_p(t), _p(p), t.numel() // 2, _p(loss), _stream()), "lp_rmse_fwd")
    return loss.reshape(())


# --------------------------------------------------------------------------------------------------------
# camera geometry of the calibrated multi-view losses (csrc/cameras.hip)
# --------------------------------------------------------------------------------------------------------

def _cam_dist12(dist: torch.Tensor) -> torch.Tensor:
    """(B, V, n) OpenCV distortion parameters, n in {4, 5, 8, 12, 14} -> (B, V, 12) fp32, missing ones 0.  The tilt pair of a 14-parameter
    set is not modelled: it must be zero (checked here, a host read that only such sets pay)."""
    n = dist.shape[-1]
    if n not in (4, 5, 8, 12, 14):
        raise ValueError(f"distortion parameters must number 4, 5, 8, 12 or 14 (OpenCV order), got {n}")
    d = _f32c(dist)
    if n == 14:
        if bool((d[..., 12:] != 0).any()):
            raise NotImplementedError("the tilted-sensor distortion parameters (tau_x, tau_y) are not implemented")
        d = d[..., :12]
    if d.shape[-1] < 12:
        d = torch.nn.functional.pad(d, (0, 12 - d.shape[-1]))
    return d.contiguous()


def _cam_rig(intrinsics: torch.Tensor, extrinsics: torch.Tensor, dist: torch.Tensor, b: int):
    if intrinsics.dim() != 4 or intrinsics.shape[0] != b or tuple(intrinsics.shape[2:]) != (3, 3):
        raise ValueError(f"intrinsics must be (batch = {b}, num_views, 3, 3), got {tuple(intrinsics.shape)}")
    v = int(intrinsics.shape[1])
    if tuple(extrinsics.shape) != (b, v, 3, 4):
        raise ValueError(f"extrinsics must be {(b, v, 3, 4)}, got {tuple(extrinsics.shape)}")
    if dist.dim() != 3 or tuple(dist.shape[:2]) != (b, v):
        raise ValueError(f"dist must be {(b, v)} + (num_params,), got {tuple(dist.shape)}")
    return _f32c(intrinsics), _f32c(extrinsics), _cam_dist12(dist), v


def _cam_bbox(bbox: torch.Tensor | None, b: int, v: int, dev: torch.device) -> torch.Tensor | None:
    if bbox is None:
        return None
    bb = _f32c(bbox).to(dev)
    if tuple(bb.shape) != (b, 4 * v):
        raise ValueError(f"bbox must be {(b, 4 * v)} ([x, y, h, w] per view), got {tuple(bb.shape)}")
    return bb


class _CamChainFn(torch.autograd.Function):
    """points (B, V, K, 2) -> p3d (B, P, K, 3) [, p2d (B, V, K, 2)]: lp_cam_chain_fwd / _bwd, one launch each"""

    @staticmethod
    def forward(ctx, points, intr, extr, dist12, bbox, mh, mw, want_2d):
        require_device(points, intr, extr, dist12, bbox)
        pts = _f32c(points)
        b, v, k, _ = pts.shape
        npairs = v * (v - 1) // 2
        p3d = torch.empty(b, npairs, k, 3, device=pts.device, dtype=torch.float32)
        p2d = torch.empty(b, v, k, 2, device=pts.device, dtype=torch.float32) if want_2d else None
        check(_lib.lib().lp_cam_chain_fwd(_p(pts), _p(intr), _p(extr), _p(dist12), _p(bbox), mh, mw, b, v, k, _p(p3d), _p(p2d), _stream()),
              "lp_cam_chain_fwd")
        ctx.save_for_backward(pts, intr, extr, dist12, p3d)
        ctx.bbox, ctx.args, ctx.in_dtype = bbox, (mh, mw), points.dtype
        ctx.set_materialize_grads(False)
        return p3d, p2d

    @staticmethod
    def backward(ctx, g3d, g2d):
        if g3d is None and g2d is None:
            return (None,) * 8
        pts, intr, extr, dist12, p3d = ctx.saved_tensors
        b, v, k, _ = pts.shape
        g3d = _f32c(g3d) if g3d is not None else None
        g2d = _f32c(g2d) if g2d is not None else None
        nws = int(_lib.lib().lp_cam_chain_workspace_bytes(b, v, k))
        ws = torch.empty(nws, device=pts.device, dtype=torch.uint8)
        gpts = torch.empty_like(pts)
        mh, mw = ctx.args
        check(_lib.lib().lp_cam_chain_bwd(_p(pts), _p(intr), _p(extr), _p(dist12), _p(ctx.bbox), mh, mw, b, v, k, _p(p3d), _p(g3d), _p(g2d),
                                          _p(ws), nws, _p(gpts), _stream()), "lp_cam_chain_bwd")
        return gpts.to(ctx.in_dtype), None, None, None, None, None, None, None


def _cam_points(points: torch.Tensor) -> tuple[int, int, int]:
    if points.dim() != 4 or points.shape[-1] != 2 or points.shape[1] < 2:
        raise ValueError(f"points must be (batch, num_views >= 2, num_keypoints, 2), got {tuple(points.shape)}")
    return int(points.shape[0]), int(points.shape[1]), int(points.shape[2])


def camera_pairs_to_3d(points: torch.Tensor, intrinsics: torch.Tensor, extrinsics: torch.Tensor, dist: torch.Tensor) -> torch.Tensor:
    """Triangulate every camera pair: points (B, V, K, 2) frame px -> (B, V (V - 1) / 2, K, 3); differentiable in the points."""
    b, v, _ = _cam_points(points)
    intr, extr, d12, v2 = _cam_rig(intrinsics, extrinsics, dist, b)
    if v2 != v:
        raise ValueError(f"{v} views of points, {v2} cameras")
    return _CamChainFn.apply(points, intr, extr, d12, None, 1.0, 1.0, False)[0]


def camera_chain(points: torch.Tensor, intrinsics: torch.Tensor, extrinsics: torch.Tensor, dist: torch.Tensor, bbox: torch.Tensor | None,
                 model_h: float, model_w: float) -> tuple[torch.Tensor, torch.Tensor]:
    """The geometry of both calibrated losses in one launch (and one backward): every pair's triangulation (B, P, K, 3), and their mean
    reprojected into every view, distorted and mapped to model px with ``bbox`` (B, 4 V) (frame px if None) -> (B, V, K, 2)."""
    b, v, _ = _cam_points(points)
    intr, extr, d12, v2 = _cam_rig(intrinsics, extrinsics, dist, b)
    if v2 != v:
        raise ValueError(f"{v} views of points, {v2} cameras")
    return _CamChainFn.apply(points, intr, extr, d12, _cam_bbox(bbox, b, v, points.device), float(model_h), float(model_w), True)


class _CamProjectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p3, intr, extr, dist12, bbox, mh, mw):
        require_device(p3, intr, extr, dist12, bbox)
        x = _f32c(p3)
        b, k, _ = x.shape
        v = intr.shape[1]
        out = torch.empty(b, v, k, 2, device=x.device, dtype=torch.float32)
        check(_lib.lib().lp_cam_project_fwd(_p(x), _p(intr), _p(extr), _p(dist12), _p(bbox), mh, mw, b, v, k, _p(out), _stream()),
              "lp_cam_project_fwd")
        ctx.save_for_backward(x, intr, extr, dist12)
        ctx.bbox, ctx.args, ctx.in_dtype = bbox, (mh, mw), p3.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        x, intr, extr, dist12 = ctx.saved_tensors
        b, k, _ = x.shape
        v = intr.shape[1]
        mh, mw = ctx.args
        gx = torch.empty_like(x)
        check(_lib.lib().lp_cam_project_bwd(_p(x), _p(intr), _p(extr), _p(dist12), _p(ctx.bbox), mh, mw, b, v, k, _p(_f32c(g)), _p(gx),
                                            _stream()), "lp_cam_project_bwd")
        return gx.to(ctx.in_dtype), None, None, None, None, None, None


def camera_project(points_3d: torch.Tensor, intrinsics: torch.Tensor, extrinsics: torch.Tensor, dist: torch.Tensor,
                   bbox: torch.Tensor | None = None, model_h: float = 1.0, model_w: float = 1.0) -> torch.Tensor:
    """points_3d (B, K, 3) -> (B, V, K, 2) in every view (frame px; model px with ``bbox``); differentiable in the points."""
    if points_3d.dim() != 3 or points_3d.shape[-1] != 3:
        raise ValueError(f"points_3d must be (batch, num_keypoints, 3), got {tuple(points_3d.shape)}")
    b = int(points_3d.shape[0])
    intr, extr, d12, v = _cam_rig(intrinsics, extrinsics, dist, b)
    return _CamProjectFn.apply(points_3d, intr, extr, d12, _cam_bbox(bbox, b, v, points_3d.device), float(model_h), float(model_w))


def pairwise_projections_loss(keypoints_targ_3d: torch.Tensor, keypoints_pred_3d: torch.Tensor) -> torch.Tensor:
    """mean over the valid (sample, pair, keypoint) of ||target - prediction||_2 (reference losses/losses.py:1036-1126); value and gradient
    in one launch, the number of valid entries never read by the host."""
    require_device(keypoints_targ_3d, keypoints_pred_3d)
    targ, pred = _f32c(keypoints_targ_3d), _f32c(keypoints_pred_3d)
    if pred.dim() != 4 or pred.shape[-1] != 3 or tuple(targ.shape) != (pred.shape[0], pred.shape[2], 3):
        raise ValueError(f"pairwise projections: predictions {tuple(pred.shape)} must be (B, pairs, K, 3) and targets (B, K, 3), got "
                         f"{tuple(targ.shape)}")
    b, npairs, k, _ = pred.shape
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    grad = torch.empty_like(pred)
    check(_lib.lib().lp_cam_pairwise_fwd_bwd(_p(targ), _p(pred), b, npairs, k, _p(loss), _p(grad), _stream()), "lp_cam_pairwise_fwd_bwd")
    return _UnitGradFn.apply(keypoints_pred_3d, loss.reshape(()), grad)


class _LossCombineFn(torch.autograd.Function):
    """weighted[i] = w[i] * x[i];  total = sum_i a[i] * weighted[i]  (csrc/kploss.hip: lp_loss_combine, one launch each way)"""

    @staticmethod
    def forward(ctx, w, a, *xs):
        n = len(xs)
        dev = xs[0].device
        weighted = torch.empty(n, device=dev, dtype=torch.float32)
        total = torch.empty((), device=dev, dtype=torch.float32)
        keep = [x.detach().reshape(1) for x in xs]   # (views of the callers' scalars: alive for the launch)
        ptrs = (C.c_void_p * n)(*[_p(x) for x in keep])
        wa, aa = (C.c_float * n)(*w), (C.c_float * n)(*a)
        check(_lib.lib().lp_loss_combine(ptrs, wa, aa, n, _p(weighted), _p(total), _stream()), "lp_loss_combine")
        ctx.w, ctx.a, ctx.n = tuple(w), tuple(a), n
        return weighted, total

    @staticmethod
    def backward(ctx, g_weighted, g_total):
        n = ctx.n
        dev = g_total.device if g_total is not None else g_weighted.device
        gx = torch.empty(n, device=dev, dtype=torch.float32)
        gw = None if g_weighted is None else _f32c(g_weighted)
        gt = None if g_total is None else _f32c(g_total)
        check(_lib.lib().lp_loss_combine_bwd((C.c_float * n)(*ctx.w), (C.c_float * n)(*ctx.a), n, _p(gw), _p(gt), _p(gx), _stream()),
              "lp_loss_combine_bwd")
        return (None, None) + tuple(gx[i] for i in range(n))


def loss_combine(losses: list[torch.Tensor], weights: list[float], anneal: list[float]) -> tuple[torch.Tensor, torch.Tensor]:
    """LossFactory's weighted sum of device scalars -> ((n,) weighted values a_l w_l x_l, 0-dim total); differentiable.  Up to 8 losses are
    one launch each way (lp_loss_combine); more - the reference's registry holds more than 8 loss classes and its factory sums any number,
    losses/factory.py:229-285 - go through groups of 8 whose totals are combined the same way."""
    require_device(*losses)
    if len(losses) == 0:
        raise ValueError("a LossFactory needs at least one loss")
    if any(x.numel() != 1 for x in losses):
        raise ValueError("every loss must be a scalar")
    xs = [x if x.dtype == torch.float32 else x.to(torch.float32) for x in losses]
    w, a = [float(v) for v in weights], [float(v) for v in anneal]
    if len(xs) <= 8:
        return _LossCombineFn.apply(w, a, *xs)
    parts = [_LossCombineFn.apply(w[i:i + 8], a[i:i + 8], *xs[i:i + 8]) for i in range(0, len(xs), 8)]
    _, total = loss_combine([p[1] for p in parts], [1.0] * len(parts), [1.0] * len(parts))
    return torch.cat([p[0] for p in parts]), total


# --------------------------------------------------------------------------------------------------------
# batch producers (csrc/frames.hip)
# --------------------------------------------------------------------------------------------------------

def _frame_norm(mean, std) -> _lib.FrameNorm:
    return _lib.FrameNorm((C.c_float * 3)(*[float(m) for m in mean]), (C.c_float * 3)(*[float(v) for v in std]))


def frames_resize(frames_u8: torch.Tensor, height: int, width: int, border: str = "clamp", mean=None, std=None,
                  interpolation: str = "linear") -> torch.Tensor:
    """(S, Hs, Ws, 3) uint8 device frames -> resized frames.  Without mean/std: fp32 (S, height, width, 3) in [0, 255] (input of
    ``frames_augment``); with them: fp32 (S, 3, height, width) normalised planes in one launch.
    ``interpolation``: "linear" = antialiased triangle filter (DALI ``fn.resize``, the video pipeline); "cubic" = bicubic without
    antialiasing, rounded to uint8 levels (imgaug ``iaa.Resize``'s default = OpenCV INTER_CUBIC, the labeled images)."""
    require_device(frames_u8)
    if interpolation not in ("linear", "cubic"):
        raise ValueError(f"interpolation must be 'linear' or 'cubic', got {interpolation!r}")
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise ValueError(f"frames must be uint8 (S, H, W, 3), got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    if border not in ("clamp", "renorm"):
        raise ValueError(f"border must be 'clamp' or 'renorm', got {border!r}")
    if frames_u8.stride(3) != 1 or frames_u8.stride(2) != 3:
        frames_u8 = frames_u8.contiguous()
    s, hs, ws, _ = frames_u8.shape
    finish = mean is not None
    out = torch.empty((s, 3, height, width) if finish else (s, height, width, 3), device=frames_u8.device, dtype=torch.float32)
    norm = _frame_norm(mean, std) if finish else None
    if interpolation == "cubic":
        check(_lib.lib().lp_frames_resize_cubic(_p(frames_u8), s, hs, ws, frames_u8.stride(0), frames_u8.stride(1), int(height), int(width), 1,
                                                C.byref(norm) if finish else None, _p(out), _stream()), "lp_frames_resize_cubic")
        return out
    check(_lib.lib().lp_frames_resize(_p(frames_u8), s, hs, ws, frames_u8.stride(0), frames_u8.stride(1), int(height), int(width),
                                      _lib.BORDER_CLAMP if border == "clamp" else _lib.BORDER_RENORM,
                                      C.byref(norm) if finish else None, _p(out), _stream()), "lp_frames_resize")
    return out


BBOX_MAX_ANCHORS, BBOX_SMOOTH_MAX_WINDOW = 64, 255   # include/lp_hip.h: LP_BBOX_MAX_ANCHORS, LP_BBOX_SMOOTH_MAX_WINDOW


def bbox_from_keypoints(keypoints: torch.Tensor, anchors: Sequence[int] = (), crop_ratio: float | None = None, crop_height: int | None = None,
                        crop_width: int | None = None) -> torch.Tensor:
    """(N, K, 2) or (N, 2K) fp32 device keypoints in frame px -> (N, 4) int32 boxes [x, y, h, w] on the device: the reference's
    ``_compute_bbox_df`` (utils/cropzoom.py:65-143) in double precision, one launch, nothing read back.  ``anchors``: keypoint indices the
    box is built from (empty: all).  Exactly one of ``crop_ratio`` and the pair (``crop_height``, ``crop_width``); frames with a non-finite
    anchor or an empty box get [0, 0, 0, 0]."""
    require_device(keypoints)
    fixed = crop_height is not None and crop_width is not None
    if fixed and crop_ratio is not None:
        raise ValueError("provide either crop_ratio or (crop_height, crop_width), not both.")
    if not fixed and crop_ratio is None:
        raise ValueError("one of crop_ratio or (crop_height, crop_width) must be provided.")
    if keypoints.dim() not in (2, 3) or (keypoints.dim() == 3 and keypoints.shape[-1] != 2) or keypoints.shape[-1] % 2 or keypoints.shape[0] == 0:
        raise ValueError(f"keypoints must be (N, K, 2) or (N, 2K), got {tuple(keypoints.shape)}")
    kp = _f32c(keypoints)
    n, k = int(kp.shape[0]), int(kp.numel() // (2 * kp.shape[0]))
    idx = [int(a) for a in anchors]
    if any(a < 0 or a >= k for a in idx):
        raise ValueError(f"anchor indices must lie in [0, {k}), got {idx}")
    out = torch.empty(n, 4, device=kp.device, dtype=torch.int32)
    arr = (C.c_int * max(1, len(idx)))(*idx)
    check(_lib.lib().lp_bbox_from_keypoints(_p(kp), n, k, arr, len(idx), 0.0 if fixed else float(crop_ratio), int(crop_height) if fixed else 0,
                                            int(crop_width) if fixed else 0, _p(out), _stream()), "lp_bbox_from_keypoints")
    return out


def bbox_smooth(bbox: torch.Tensor, window: int) -> torch.Tensor:
    """(N, 4) int32 device boxes -> their centred rolling median (pandas ``rolling(window, center=True, min_periods=1).median().round(0)``,
    utils/cropzoom.py:391-392), (N, 4) int32.  ``window`` above ``BBOX_SMOOTH_MAX_WINDOW`` is refused (NotImplementedError)."""
    require_device(bbox)
    if bbox.dtype != torch.int32 or bbox.dim() != 2 or bbox.shape[1] != 4 or bbox.shape[0] == 0:
        raise ValueError(f"bbox must be int32 (N, 4), got {bbox.dtype} {tuple(bbox.shape)}")
    if int(window) < 1:
        raise ValueError(f"window must be at least 1, got {window}")
    bb = bbox.contiguous()
    out = torch.empty_like(bb)
    check(_lib.lib().lp_bbox_smooth(_p(bb), int(bb.shape[0]), int(window), _p(out), _stream()), "lp_bbox_smooth")
    return out


def frames_crop_resize(frames_u8: torch.Tensor, bbox: torch.Tensor, height: int, width: int, mean, std, border: str = "clamp") -> torch.Tensor:
    """(S, Hs, Ws, 3) uint8 device frames + (S, 4) int32 device boxes [x, y, h, w] -> fp32 (S, 3, height, width) normalised planes of each
    frame's own box, in one launch: bit-identical to ``frames_resize(crop, height, width, border, mean, std)`` of the zero-padded crop."""
    require_device(frames_u8, bbox)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise ValueError(f"frames must be uint8 (S, H, W, 3), got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    if border not in ("clamp", "renorm"):
        raise ValueError(f"border must be 'clamp' or 'renorm', got {border!r}")
    if bbox.dtype != torch.int32 or tuple(bbox.shape) != (frames_u8.shape[0], 4):
        raise ValueError(f"bbox must be int32 ({frames_u8.shape[0]}, 4), got {bbox.dtype} {tuple(bbox.shape)}")
    if frames_u8.stride(3) != 1 or frames_u8.stride(2) != 3:
        frames_u8 = frames_u8.contiguous()
    s, hs, ws, _ = frames_u8.shape
    bb = bbox.contiguous()
    out = torch.empty((s, 3, int(height), int(width)), device=frames_u8.device, dtype=torch.float32)
    norm = _frame_norm(mean, std)
    check(_lib.lib().lp_frames_crop_resize(_p(frames_u8), s, hs, ws, frames_u8.stride(0), frames_u8.stride(1), _p(bb), int(height), int(width),
                                           _lib.BORDER_CLAMP if border == "clamp" else _lib.BORDER_RENORM, C.byref(norm), _p(out), _stream()),
          "lp_frames_crop_resize")
    return out


def frames_augment(frames_hwc: torch.Tensor, mean, std, matrix=None, brightness: float = 1.0, contrast: float = 1.0,
                   contrast_center: float = 0.5, shot_factor: float = 0.0, seed: int = 0) -> torch.Tensor:
    """fp32 (S, H, W, 3) in [0, 255] -> warp_affine(matrix: source -> destination, fill 0) -> brightness / contrast -> shot
    noise -> /255 -> normalise -> fp32 (S, 3, H, W).  ``matrix`` is a host (2, 3) array-like (one DALI sample = one sequence)."""
    require_device(frames_hwc)
    x = _f32c(frames_hwc)
    s, h, w, c = x.shape
    if c != 3:
        raise ValueError(f"frames must be (S, H, W, 3), got {tuple(x.shape)}")
    m = [0.0] * 6 if matrix is None else [float(v) for v in np.asarray(matrix, dtype=np.float64).reshape(-1)]
    if len(m) != 6:
        raise ValueError("matrix must have 6 entries (2, 3)")
    aug = _lib.FrameAugment(int(matrix is not None), (C.c_float * 6)(*m), float(brightness), float(contrast), float(contrast_center),
                            float(shot_factor), int(seed) & 0xFFFFFFFFFFFFFFFF)
    norm = _frame_norm(mean, std)
    out = torch.empty(s, 3, h, w, device=x.device, dtype=torch.float32)
    check(_lib.lib().lp_frames_augment(_p(x), s, h, w, C.byref(aug), C.byref(norm), _p(out), _stream()), "lp_frames_augment")
    return out


def labeled_keypoints(keypoints: torch.Tensor, src_hw: torch.Tensor, height: int, width: int, affine: torch.Tensor | None = None,
                      hflip: torch.Tensor | None = None, swap: torch.Tensor | None = None, visibility: torch.Tensor | None = None,
                      uniform_heatmaps: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """(B, K, 2) source-px labels -> (model-px keypoints with out-of-frame points NaN, visibility (B, K) int32)."""
    require_device(keypoints)
    kp = _f32c(keypoints)
    b, k, _ = kp.shape
    dev = kp.device
    hw = _f32c(src_hw.to(dev))
    i32 = lambda t: None if t is None else t.to(device=dev, dtype=torch.int32).contiguous()  # noqa: E731
    aff = None if affine is None else _f32c(affine.to(dev))
    fl, sw, vi = i32(hflip), i32(swap), i32(visibility)
    if hw.shape != (b, 2) or (aff is not None and aff.shape != (b, 2, 3)) or (sw is not None and sw.numel() != k):
        raise ValueError("labeled_keypoints: src_hw must be (B, 2), affine (B, 2, 3), swap (K,)")
    out = torch.empty_like(kp)
    vis = torch.empty(b, k, device=dev, dtype=torch.int32)
    check(_lib.lib().lp_labeled_keypoints(_p(kp), _p(hw), _p(aff), _p(fl), _p(sw), _p(vi), int(uniform_heatmaps), b, k, int(height),
                                          int(width), _p(out), _p(vis), _stream()), "lp_labeled_keypoints")
    return out, vis


# --------------------------------------------------------------------------------------------------------
# multi-view labeled batches with the 3-D augmentation (csrc/mv3d.hip)
# --------------------------------------------------------------------------------------------------------

MV3D_MAX_VIEWS, MV3D_MAX_KEYPOINTS = 8, 128   # include/lp_hip.h: LP_MV3D_MAX_VIEWS, LP_MV3D_MAX_KEYPOINTS


def mv3d_plan(keypoints: torch.Tensor, src_hw: torch.Tensor, bbox: torch.Tensor, intrinsics: torch.Tensor, extrinsics: torch.Tensor,
              dist: torch.Tensor, draws: torch.Tensor, height: int, width: int, augment: bool = True, shift_param: float = 0.25
              ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """One launch for the batch: labels (B, V, K, 2) in stored-image px -> triangulation, 3-D scale and translation from ``draws`` (B, 4) =
    [scale, r_x, r_y, r_z], reprojection and the per-view similarity (include/lp_hip.h: lp_mv3d_plan).  Returns ``kp3d`` (B, K, 3), ``kp2d``
    (B, V, K, 2) in model px, ``affine`` (B, V, 2, 3) stored px -> warped px, ``status`` (B) int32 (0 augmented, 1 not augmented, 2 no label at
    all, 3 a view with fewer than 3 matched keypoints: not augmented).  Nothing is read back."""
    require_device(keypoints, src_hw, bbox, intrinsics, extrinsics, dist, draws)
    b, v, k = _cam_points(keypoints)
    intr, extr, d12, v2 = _cam_rig(intrinsics, extrinsics, dist, b)
    if v2 != v:
        raise ValueError(f"{v} views of keypoints, {v2} cameras")
    dev = keypoints.device
    kp, hw, dr = _f32c(keypoints), _f32c(src_hw).to(dev), _f32c(draws).to(dev)
    bb = _cam_bbox(bbox, b, v, dev)
    if bb is None or tuple(hw.shape) != (b, v, 2) or tuple(dr.shape) != (b, 4):
        raise ValueError(f"mv3d_plan: bbox must be {(b, 4 * v)}, src_hw {(b, v, 2)} and draws {(b, 4)}, got "
                         f"{None if bbox is None else tuple(bbox.shape)}, {tuple(hw.shape)}, {tuple(dr.shape)}")
    kp3d = torch.empty(b, k, 3, device=dev, dtype=torch.float32)
    kp2d = torch.empty(b, v, k, 2, device=dev, dtype=torch.float32)
    affine = torch.empty(b, v, 2, 3, device=dev, dtype=torch.float32)
    status = torch.empty(b, device=dev, dtype=torch.int32)
    check(_lib.lib().lp_mv3d_plan(_p(kp), _p(hw), _p(bb), _p(intr), _p(extr), _p(d12), _p(dr), int(bool(augment)), float(shift_param), int(height),
                                  int(width), b, v, k, _p(kp3d), _p(kp2d), _p(affine), _p(status), _stream()), "lp_mv3d_plan")
    return kp3d, kp2d, affine, status


def _mv3d_images(images_u8: torch.Tensor) -> torch.Tensor:
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise ValueError(f"images must be uint8 (B, H, W, 3), got {images_u8.dtype} {tuple(images_u8.shape)}")
    return images_u8.contiguous()


def mv3d_fill(images_u8: torch.Tensor, mean, std) -> torch.Tensor:
    """(B, Hs, Ws, 3) uint8 -> (B,) the smallest normalised pixel value of each image (what the reference pads the warped image with)."""
    require_device(images_u8)
    src = _mv3d_images(images_u8)
    b, hs, ws, _ = src.shape
    fill = torch.empty(b, device=src.device, dtype=torch.float32)
    check(_lib.lib().lp_mv3d_fill(_p(src), b, hs, ws, C.byref(_frame_norm(mean, std)), _p(fill), _stream()), "lp_mv3d_fill")
    return fill


def mv3d_finish(images_u8: torch.Tensor, affine: torch.Tensor, fill: torch.Tensor, mean, std, view: int, out: torch.Tensor) -> torch.Tensor:
    """One view's (B, Hs, Ws, 3) uint8 images -> normalise, warp by ``affine[:, view]`` (B, V, 2, 3; stored px -> warped px), resize to
    ``out``'s (H, W): written straight into ``out[:, view]`` of the fp32 (B, V, 3, H, W) batch (include/lp_hip.h: lp_mv3d_finish)."""
    require_device(images_u8, affine, fill, out)
    src = _mv3d_images(images_u8)
    b, hs, ws, _ = src.shape
    if out.dim() != 5 or out.dtype != torch.float32 or not out.is_contiguous() or out.shape[0] != b or out.shape[2] != 3:
        raise ValueError(f"out must be contiguous fp32 ({b}, V, 3, H, W), got {out.dtype} {tuple(out.shape)}")
    v, h, w = int(out.shape[1]), int(out.shape[3]), int(out.shape[4])
    if affine.dtype != torch.float32 or not affine.is_contiguous() or tuple(affine.shape) != (b, v, 2, 3):
        raise ValueError(f"affine must be contiguous fp32 {(b, v, 2, 3)}, got {affine.dtype} {tuple(affine.shape)}")
    if fill.dtype != torch.float32 or not fill.is_contiguous() or tuple(fill.shape) != (b,):
        raise ValueError(f"fill must be contiguous fp32 {(b,)}, got {fill.dtype} {tuple(fill.shape)}")
    if not 0 <= int(view) < v:
        raise ValueError(f"view {view} outside [0, {v})")
    check(_lib.lib().lp_mv3d_finish(_p(src), b, hs, ws, _p(affine), _p(fill), C.byref(_frame_norm(mean, std)), v, int(view), h, w, _p(out),
                                    _stream()), "lp_mv3d_finish")
    return out


# --------------------------------------------------------------------------------------------------------
# labeled-frame augmentation (csrc/labelaug.hip): one parameter table per batch, one launch sequence per stage
# --------------------------------------------------------------------------------------------------------

# include/lp_hip.h: lp_labelaug_image, field for field (60 four-byte words)
LABELAUG_DTYPE = np.dtype([("flags", "<i4"), ("image_id", "<i4"), ("geom", "<f4", (6,)), ("blur", "<f4", (25,)), ("emboss", "<f4", (9,)),
                           ("coarse_gh", "<i4", (3,)), ("coarse_gw", "<i4", (3,)), ("coarse_thr", "<u4", (3,)), ("elastic_alpha", "<f4"),
                           ("clahe_clip", "<i4"), ("clahe_tiles_y", "<i4"), ("clahe_tiles_x", "<i4"), ("clahe_slot", "<i4"),
                           ("pad", "<i4", (4,))])
assert LABELAUG_DTYPE.itemsize == 60 * 4


def salt_quantiles() -> np.ndarray:
    """The 256-entry quantile table of the value imgaug's CoarseSalt writes, 255 (0.5 + |Beta(0.5, 0.5) - 0.5|) = 127.5 + 127.5 |cos(pi u)|
    at u = (i + 0.5) / 256 (CoarsePepper: 255 minus it)."""
    u = (np.arange(256) + 0.5) / 256.0
    return np.floor(127.5 + 127.5 * np.abs(np.cos(np.pi * u)) + 0.5).clip(0, 255).astype(np.uint8)


def labelaug_table(table: np.ndarray, device) -> torch.Tensor:
    """host parameter table (LABELAUG_DTYPE, one row per image) -> the device bytes the labelaug_* wrappers take"""
    if table.dtype != LABELAUG_DTYPE or table.ndim != 1:
        raise ValueError(f"table must be a 1-D array of ops.LABELAUG_DTYPE, got {table.dtype} {table.shape}")
    return torch.from_numpy(np.ascontiguousarray(table).view(np.uint8).copy()).to(device)


def _aug_images(images_u8: torch.Tensor, table: torch.Tensor) -> tuple[torch.Tensor, int, int, int]:
    require_device(images_u8, table)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise ValueError(f"images must be uint8 (B, H, W, 3), got {images_u8.dtype} {tuple(images_u8.shape)}")
    b, h, w, _ = images_u8.shape
    if table.dtype != torch.uint8 or table.numel() != b * LABELAUG_DTYPE.itemsize:
        raise ValueError(f"table must hold {b} rows of {LABELAUG_DTYPE.itemsize} bytes (ops.labelaug_table)")
    return images_u8.contiguous(), b, h, w


def labelaug_geom(images_u8: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """Rot90 + Affine: one bilinear gather through the table's destination -> source maps (fill 0)"""
    x, b, h, w = _aug_images(images_u8, table)
    out = torch.empty_like(x)
    check(_lib.lib().lp_labelaug_geom(_p(x), b, h, w, _p(table), _p(out), _stream()), "lp_labelaug_geom")
    return out


def labelaug_local(images_u8: torch.Tensor, table: torch.Tensor, which: int, seed: int = 0, salt_lut: torch.Tensor | None = None) -> torch.Tensor:
    """which = _lib.AUG_LOCAL_BLUR_COARSE: MotionBlur -> CoarseDropout -> CoarseSalt -> CoarsePepper; _lib.AUG_LOCAL_EMBOSS: Emboss"""
    x, b, h, w = _aug_images(images_u8, table)
    if which == _lib.AUG_LOCAL_BLUR_COARSE and salt_lut is None:
        salt_lut = torch.from_numpy(salt_quantiles()).to(x.device)
    out = torch.empty_like(x)
    check(_lib.lib().lp_labelaug_local(_p(x), b, h, w, _p(table), int(which), _p(salt_lut), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(out),
                                       _stream()), "lp_labelaug_local")
    return out


def labelaug_elastic_field(table: torch.Tensor, b: int, h: int, w: int, sigma: float, seed: int = 0) -> torch.Tensor:
    """fp32 (B, 2, H, W) displacement (dx, dy) of the images whose ELASTIC flag is set (zero elsewhere)"""
    require_device(table)
    tmp = torch.empty(b, 2, h, w, device=table.device, dtype=torch.float32)
    field = torch.zeros(b, 2, h, w, device=table.device, dtype=torch.float32)
    check(_lib.lib().lp_labelaug_elastic_field(int(b), int(h), int(w), _p(table), float(sigma), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(tmp),
                                               _p(field), _stream()), "lp_labelaug_elastic_field")
    return field


def labelaug_elastic_apply(images_u8: torch.Tensor, table: torch.Tensor, field: torch.Tensor) -> torch.Tensor:
    """out(x, y) = bicubic sample of the image at (x + dx, y + dy), zero outside"""
    x, b, h, w = _aug_images(images_u8, table)
    f = _f32c(field)
    if f.shape != (b, 2, h, w):
        raise ValueError(f"field must be (B, 2, H, W) = {(b, 2, h, w)}, got {tuple(f.shape)}")
    out = torch.empty_like(x)
    check(_lib.lib().lp_labelaug_elastic_apply(_p(x), b, h, w, _p(table), _p(f), _p(out), _stream()), "lp_labelaug_elastic_apply")
    return out


def labelaug_histeq(images_u8: torch.Tensor, table: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """AllChannelsHistogramEqualization -> (images, the (B, 3, 256) uint8 look-up tables; rows of images without the flag are zero)"""
    x, b, h, w = _aug_images(images_u8, table)
    ws = torch.empty(b * 768, device=x.device, dtype=torch.int32)
    lut = torch.zeros(b, 3, 256, device=x.device, dtype=torch.uint8)
    out = torch.empty_like(x)
    check(_lib.lib().lp_labelaug_histeq(_p(x), b, h, w, _p(table), _p(ws), _p(lut), _p(out), _stream()), "lp_labelaug_histeq")
    return out, lut


def labelaug_clahe(images_u8: torch.Tensor, table: torch.Tensor, slot_image: Sequence[int], max_ty: int, max_tx: int) -> torch.Tensor:
    """AllChannelsCLAHE; ``slot_image[s]`` = the image whose table row says ``clahe_slot == s`` (host knowledge: no read-back)"""
    x, b, h, w = _aug_images(images_u8, table)
    n = len(slot_image)
    slots = torch.tensor(list(slot_image), dtype=torch.int32).to(x.device) if n else None
    luts = torch.empty(max(n, 1) * max(max_ty, 1) * max(max_tx, 1) * 768, device=x.device, dtype=torch.uint8)
    out = torch.empty_like(x)
    check(_lib.lib().lp_labelaug_clahe(_p(x), b, h, w, _p(table), _p(slots), n, int(max_ty), int(max_tx), _p(luts), _p(out), _stream()),
          "lp_labelaug_clahe")
    return out


def labelaug_finish(images_u8: torch.Tensor, table: torch.Tensor, height: int, width: int, mean, std) -> torch.Tensor:
    """CropAndPad -> cubic Resize -> /255 -> normalise -> optional mirror: fp32 (B, 3, height, width)"""
    x, b, hs, ws = _aug_images(images_u8, table)
    norm = _frame_norm(mean, std)
    out = torch.empty(b, 3, int(height), int(width), device=x.device, dtype=torch.float32)
    check(_lib.lib().lp_labelaug_finish(_p(x), b, hs, ws, _p(table), int(height), int(width), C.byref(norm), _p(out), _stream()),
          "lp_labelaug_finish")
    return out


def labelaug_keypoints(keypoints: torch.Tensor, affine: torch.Tensor | None, table: torch.Tensor | None, field: torch.Tensor | None,
                       h: int, w: int) -> torch.Tensor:
    """(B, K, 2) source-px labels through the (B, 2, 3) affine of Rot90 / Affine and, with ``field``, the elastic displacement"""
    require_device(keypoints)
    kp = _f32c(keypoints)
    b, k, _ = kp.shape
    aff = None if affine is None else _f32c(affine.to(kp.device))
    if aff is not None and aff.shape != (b, 2, 3):
        raise ValueError("labelaug_keypoints: affine must be (B, 2, 3)")
    f = None if field is None else _f32c(field)
    if f is not None and (f.shape != (b, 2, h, w) or table is None):
        raise ValueError("labelaug_keypoints: field must be (B, 2, H, W) and comes with its table")
    out = torch.empty_like(kp)
    check(_lib.lib().lp_labelaug_keypoints(_p(kp), b, k, _p(aff), _p(table), _p(f), int(h), int(w), _p(out), _stream()),
          "lp_labelaug_keypoints")
    return out


# --------------------------------------------------------------------------------------------------------
# patch masking (csrc/patchmask.hip): the multi-view transformer's curriculum, one launch per batch
# --------------------------------------------------------------------------------------------------------

PATCH_MASK_MAX_PATCHES = 1024   # csrc/patchmask.hip: kPatchMaskMaxN


def patch_mask_key(seed: int, step: int) -> int:
    """the Philox key of a (seed, training step): (seed mod 2^32) | (step mod 2^32) << 32"""
    return (int(seed) & 0xFFFFFFFF) | ((int(step) & 0xFFFFFFFF) << 32)


def patch_mask(images: torch.Tensor, key: int | tuple[int, int], count: int, patch: int = 16,
               mask: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``images`` (B, V, C, H, W) fp32 -> (the images with ``count`` patches of every view set to +0.0, the (B, V, N) fp32 mask of 1 = kept /
    0 = masked), N = (H // patch) * (W // patch).  ``key``: the 64-bit Philox key, or ``(seed, step)`` for ``patch_mask_key``.  The choice is
    the rank rule of include/lp_hip.h (lp_patch_mask_f32): a function of (key, b * V + v, patch) alone.  ``mask`` (B, V, N), 0 = mask: used
    as given instead of choosing, ``count`` is then ignored.  One launch, nothing comes back to the host; ``images`` is not written."""
    assert not images.requires_grad, "patch_mask has no backward: images carry no gradient"
    require_device(images, mask)
    if images.dim() != 5 or images.dtype != torch.float32:
        raise ValueError(f"images must be fp32 (B, V, C, H, W), got {images.dtype} {tuple(images.shape)}")
    b, v, c, h, w = images.shape
    patch = int(patch)
    n = (h // patch) * (w // patch) if patch > 0 else 0
    if n > PATCH_MASK_MAX_PATCHES:
        raise NotImplementedError(f"patch_mask: {h} x {w} px at patch {patch} is {n} patches per view; the kernel ranks at most "
                                  f"{PATCH_MASK_MAX_PATCHES} (512 x 512 px at patch 16)")
    x = images.contiguous()
    given = None
    if mask is not None:
        if tuple(mask.shape) != (b, v, n):
            raise ValueError(f"mask must be (B, V, N) = {(b, v, n)}, got {tuple(mask.shape)}")
        given = _f32c(mask)
    if isinstance(key, tuple):
        key = patch_mask_key(*key)
    out = torch.empty_like(x)
    mask_out = torch.empty(b, v, n, device=x.device, dtype=torch.float32)
    check(_lib.lib().lp_patch_mask_f32(_p(x), b * v, c, h, w, patch, int(count), int(key) & 0xFFFFFFFFFFFFFFFF, _p(given), _p(out), _p(mask_out),
                                       _stream()), "lp_patch_mask_f32")
    return out, mask_out
