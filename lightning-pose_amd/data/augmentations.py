"""Augmentation of the labeled frames on the device: the imgaug vocabulary of the reference's ``lightning_pose/data/augmentations.py``
(``imgaug_transform`` :25-119, ``expand_imgaug_str_to_dict`` :122-240) with ``csrc/labelaug.hip`` underneath.

``expand_imgaug_str_to_dict``  the six preset strings -> the reference's parameter dictionaries (same keys, order, probabilities, ranges)
``imgaug_transform``           a parameter dictionary -> ``LabeledAugmentation``, this project's pipeline object (where the reference returns
                               an ``iaa.Sequential``): it DRAWS one parameter table per batch on the host and RUNS the batch through a fixed
                               number of kernel launches; ``LabeledBatchProducer(..., augment=...)`` finishes with crop-and-pad, the cubic
                               resize, normalisation and the optional flip, and carries the keypoints through the same geometry.

imgaug and OpenCV are not available to check against: the operators restate imgaug 0.4's documented definitions, pixel parity with imgaug
itself is UNPINNED (the conventions chosen are listed at the top of ``csrc/labelaug.hip`` and in DESIGN.md).  Nothing is skipped silently: an
operator that is not implemented, a keyword of an implemented operator that is not honoured, or an order of operators that the stage layout
cannot express raises ``NotImplementedError`` naming the offender.

Stage layout (one launch sequence per stage for the whole batch, operators in the dictionary's order):
    geom     Rot90 -> Affine                                          one bilinear gather
    local    MotionBlur -> CoarseDropout -> CoarseSalt -> CoarsePepper  one stencil pass
    elastic  ElasticTransformation                                    noise + separable Gaussian (2 launches), bicubic gather
    histeq   AllChannelsHistogramEqualization                         histogram, table, apply
    clahe    AllChannelsCLAHE                                         per-tile tables, blended apply
    emboss   Emboss                                                   one stencil pass
    croppad  CropAndPad (keep_size=False, last)                       fused into the final resize
"""

from __future__ import annotations

import math
import os
from typing import Any

import numpy as np
import torch

from .. import _lib, ops

_ALLOWED_IMGAUG_STRS = ["default", "none", "dlc", "dlc-lr", "dlc-top-down", "dlc-mv"]


def expand_imgaug_str_to_dict(params: str) -> dict[str, Any]:
    """Preset string -> parameter dictionary (transform name -> {"p", "kwargs"}), as the reference expands it."""
    if params not in _ALLOWED_IMGAUG_STRS:
        raise NotImplementedError(f"cfg.training.imgaug string {params} must be in {_ALLOWED_IMGAUG_STRS}")
    out: dict[str, Any] = {}
    if params in ("default", "none"):
        return out  # resize only
    planar = not params.endswith("mv")  # the multiview preset keeps no per-view 2-D geometry
    if params == "dlc-lr":
        out["Rot90"] = {"p": 1.0, "kwargs": {"k": [[0, 2]]}}
    if params == "dlc-top-down":
        out["Rot90"] = {"p": 1.0, "kwargs": {"k": [[0, 1, 2, 3]]}}
    if planar:
        out["Affine"] = {"p": 0.4, "kwargs": {"rotate": (-25, 25)}}
    out["MotionBlur"] = {"p": 0.5, "kwargs": {"k": 5, "angle": (-90, 90)}}
    out["CoarseDropout"] = {"p": 0.5, "kwargs": {"p": 0.02, "size_percent": 0.3, "per_channel": 0.5}}
    out["CoarseSalt"] = {"p": 0.5, "kwargs": {"p": 0.01, "size_percent": (0.05, 0.1)}}
    out["CoarsePepper"] = {"p": 0.5, "kwargs": {"p": 0.01, "size_percent": (0.05, 0.1)}}
    if planar:
        out["ElasticTransformation"] = {"p": 0.5, "kwargs": {"alpha": (0, 10), "sigma": 5}}
    out["AllChannelsHistogramEqualization"] = {"p": 0.1, "kwargs": {}}
    out["AllChannelsCLAHE"] = {"p": 0.1, "kwargs": {}}
    out["Emboss"] = {"p": 0.1, "kwargs": {"alpha": (0, 0.5), "strength": (0.5, 1.5)}}
    if planar:
        out["CropAndPad"] = {"p": 0.4, "kwargs": {"percent": (-0.15, 0.15), "keep_size": False}}
    return out


# operator -> (stage, rank inside the stage, keywords that are honoured)
_OPS = {
    "Rot90": ("geom", 0, {"k", "keep_size"}),
    "Affine": ("geom", 1, {"rotate", "scale", "translate_percent"}),
    "MotionBlur": ("local", 0, {"k", "angle", "direction"}),
    "CoarseDropout": ("local", 1, {"p", "size_percent", "per_channel"}),
    "CoarseSalt": ("local", 2, {"p", "size_percent"}),
    "CoarsePepper": ("local", 3, {"p", "size_percent"}),
    "ElasticTransformation": ("elastic", 0, {"alpha", "sigma"}),
    "AllChannelsHistogramEqualization": ("histeq", 0, set()),
    "AllChannelsCLAHE": ("clahe", 0, {"clip_limit", "tile_grid_size_px"}),
    "Emboss": ("emboss", 0, {"alpha", "strength"}),
    "CropAndPad": ("croppad", 0, {"percent", "keep_size"}),
}
GEOMETRIC_OPS = ("Rot90", "Affine", "ElasticTransformation", "CropAndPad")
# imgaug 0.4 defaults the presets rely on
_DEFAULTS = {
    "Rot90": {"k": 1, "keep_size": True},
    "Affine": {"rotate": 0.0, "scale": 1.0, "translate_percent": 0.0},
    "MotionBlur": {"k": (3, 7), "angle": (0, 360), "direction": (-1.0, 1.0)},
    "CoarseDropout": {"p": (0.02, 0.1), "size_percent": None, "per_channel": False},
    "CoarseSalt": {"p": (0.02, 0.1), "size_percent": None},
    "CoarsePepper": {"p": (0.02, 0.1), "size_percent": None},
    "ElasticTransformation": {"alpha": (1.0, 40.0), "sigma": (4.0, 8.0)},
    "AllChannelsHistogramEqualization": {},
    "AllChannelsCLAHE": {"clip_limit": (0.1, 8), "tile_grid_size_px": (3, 12)},
    "Emboss": {"alpha": (0.0, 1.0), "strength": (0.25, 1.0)},
    "CropAndPad": {"percent": None, "keep_size": True},
}


def _sample(rng: np.random.Generator, spec, integer: bool = False):
    """imgaug's parameter shorthand: a number is itself, a tuple (a, b) is uniform on [a, b] (integers: a..b inclusive), a list is a choice"""
    if isinstance(spec, tuple):
        a, b = spec
        return int(rng.integers(int(a), int(b) + 1)) if integer else float(rng.uniform(float(a), float(b)))
    if isinstance(spec, list):
        v = spec[int(rng.integers(len(spec)))]
        return int(v) if integer else float(v)
    return int(spec) if integer else float(spec)


def _t(tx: float, ty: float) -> np.ndarray:
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def rot90_matrix(k: int, h: int, w: int) -> np.ndarray:
    """k quarter turns clockwise of an (h, w) image, scaled back to (h, w): source -> destination on continuous coordinates"""
    k = int(k) % 4
    if k == 0:
        return np.eye(3)
    if k == 2:
        return np.array([[-1.0, 0.0, w], [0.0, -1.0, h], [0.0, 0.0, 1.0]])
    turn = np.array([[0.0, -1.0, h], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) if k == 1 else np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, w], [0.0, 0.0, 1.0]])
    return np.diag([w / h, h / w, 1.0]) @ turn  # the turned image is (w, h): back to (h, w)


def affine_matrix(rotate_deg: float, scale: float, translate_percent: tuple[float, float], h: int, w: int) -> np.ndarray:
    """imgaug ``Affine`` about the image centre: scale, rotate (positive = clockwise on the screen), translate; source -> destination"""
    th = math.radians(rotate_deg)
    rot = np.array([[math.cos(th), -math.sin(th), 0.0], [math.sin(th), math.cos(th), 0.0], [0.0, 0.0, 1.0]])
    return _t(w / 2.0 + translate_percent[0] * w, h / 2.0 + translate_percent[1] * h) @ rot @ np.diag([scale, scale, 1.0]) @ _t(-w / 2.0, -h / 2.0)


def motion_blur_weights_batch(k: np.ndarray, angle_deg: np.ndarray, direction: np.ndarray) -> np.ndarray:
    """imgaug ``MotionBlur`` for n images at once -> (n, 5, 5): a k x k image whose centre column holds linspace(d, 1 - d), d = (direction + 1)
    / 2, as uint8 levels, rotated by ``angle`` about its centre (Affine: bilinear, fill 0, positive = clockwise on the screen), rounded to
    levels again and normalised to sum 1 - embedded in the 5 x 5 weights of the stencil kernel."""
    k, angle_deg, direction = np.asarray(k, dtype=np.int64), np.asarray(angle_deg, dtype=np.float64), np.asarray(direction, dtype=np.float64)
    out = np.zeros((len(k), 5, 5))
    for kk in (3, 5):
        sel = np.nonzero(k == kk)[0]
        if not len(sel):
            continue
        d = (np.clip(direction[sel], -1.0, 1.0) + 1.0) / 2.0
        m = np.zeros((len(sel), kk, kk))
        m[:, :, kk // 2] = np.floor((d[:, None] + (1.0 - 2.0 * d[:, None]) * np.linspace(0.0, 1.0, kk)[None]) * 255.0 + 0.5)
        th = np.radians(angle_deg[sel])[:, None, None]
        ys, xs = np.mgrid[0:kk, 0:kk]
        u, v = xs[None] + 0.5 - kk / 2.0, ys[None] + 0.5 - kk / 2.0          # destination pixel centres about the centre
        sx = np.cos(th) * u + np.sin(th) * v + kk / 2.0 - 0.5                  # through the inverse rotation: source pixel indices
        sy = -np.sin(th) * u + np.cos(th) * v + kk / 2.0 - 0.5
        x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
        ax, ay = sx - x0, sy - y0
        n = np.arange(len(sel))[:, None, None]
        acc = np.zeros_like(sx)
        for dy, wy in ((0, 1.0 - ay), (1, ay)):
            for dx, wx in ((0, 1.0 - ax), (1, ax)):
                xi, yi = x0 + dx, y0 + dy
                ok = (xi >= 0) & (xi < kk) & (yi >= 0) & (yi < kk)
                acc += np.where(ok, m[n, np.clip(yi, 0, kk - 1), np.clip(xi, 0, kk - 1)], 0.0) * wx * wy
        acc = np.floor(acc + 0.5) / 255.0
        o = (5 - kk) // 2
        out[sel, o:o + kk, o:o + kk] = acc / acc.sum((1, 2), keepdims=True)   # (the centre pixel keeps its weight: the sum is never 0)
    return out


def motion_blur_weights(k: int, angle_deg: float, direction: float) -> np.ndarray:
    """one image's 5 x 5 MotionBlur weights (see ``motion_blur_weights_batch``)"""
    return motion_blur_weights_batch(np.array([k]), np.array([angle_deg]), np.array([direction]))[0]


def emboss_weights(alpha, strength) -> np.ndarray:
    """imgaug ``Emboss``: (1 - alpha) identity + alpha [[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]]; arrays of n values give (n, 3, 3)"""
    a, s = np.asarray(alpha, dtype=np.float64)[..., None, None], np.asarray(strength, dtype=np.float64)[..., None, None]
    base = np.array([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    ramp = np.array([[-1.0, -1.0, 0.0], [-1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    same = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    return (1.0 - a) * same + a * (base + s * ramp)


def clahe_geometry(h: int, w: int, tiles, clip_limit):
    """(tiles_y, tiles_x, clip count) of one image or of n.  A CHOSEN reading: imgaug names the parameter ``tile_grid_size_px`` and documents
    it as a size in pixels, but hands the sampled value to OpenCV as ``tileGridSize``, which is the NUMBER of tiles per side (3..12 by
    default) - that reading is taken here (the other one, tiles of 3..12 px, would turn the operator into a local rank transform).  OpenCV
    clips every bin at max(1, int(clip_limit * tile area / 256))."""
    ty, tx = np.clip(np.asarray(tiles, dtype=np.int64), 1, h), np.clip(np.asarray(tiles, dtype=np.int64), 1, w)
    area = (-(-h // ty)) * (-(-w // tx))
    clip = np.maximum(1, (np.asarray(clip_limit, dtype=np.float64) * area / 256.0).astype(np.int64))
    return (int(ty), int(tx), int(clip)) if np.ndim(tiles) == 0 else (ty, tx, clip)


def _sample_n(rng: np.random.Generator, spec, n: int, integer: bool = False) -> np.ndarray:
    """``_sample`` for n images with ONE generator call"""
    if isinstance(spec, tuple):
        return rng.integers(int(spec[0]), int(spec[1]) + 1, size=n) if integer else rng.uniform(float(spec[0]), float(spec[1]), size=n)
    if isinstance(spec, list):
        return np.asarray(spec, dtype=np.int64 if integer else np.float64)[rng.integers(len(spec), size=n)]
    return np.full(n, int(spec) if integer else float(spec))


class LabeledAugmentation:
    """A device augmentation pipeline for labeled frames.  ``len()`` counts its operators (0 = resize only).

    ``draw(b, h, w)`` makes every per-image decision for one batch on the host: {"table": the ``ops.LABELAUG_DTYPE`` rows the kernels read,
    "affine": (b, 3, 3) float64 source -> destination matrices of Rot90 and Affine, "seed": the Philox key of the batch, "raw": the sampled
    parameters by name (NaN where the operator is off), "pipeline": this object}.  The generator is ``np.random.default_rng(seed + LOCAL_RANK)``, as for the video
    pipeline; the same seed gives bit-identical batches, and a draw can be replayed through ``LabeledBatchProducer(..., augment=draw)``."""

    def __init__(self, operators: list[tuple[str, float, dict]], seed: int = 123456) -> None:
        self.operators = operators
        self.names = [n for n, _, _ in operators]
        stages: list[str] = []
        last_rank = -1
        for i, name in enumerate(self.names):
            stage, rank, _ = _OPS[name]
            if stages and stages[-1] == stage and rank > last_rank:
                pass
            elif stage in stages:
                raise NotImplementedError(f"{name}: this order of operators is not expressible in the stage layout (stage '{stage}' would run "
                                          f"twice; see lightning_pose_amd.data.augmentations)")
            else:
                stages.append(stage)
            last_rank = rank
            if stage == "geom" and "elastic" in stages:
                raise NotImplementedError(f"{name} after ElasticTransformation is not expressible: the keypoints go through Rot90 / Affine first and "
                                          "the elastic field second (put ElasticTransformation after the affine operators)")
            if name == "CropAndPad" and i != len(self.names) - 1:
                raise NotImplementedError("CropAndPad changes the image size and is fused into the final resize: it must be the last operator")
        self.stages = stages
        self.elastic_sigma = None
        for name, _, kw in operators:
            if name == "ElasticTransformation":
                sigma = kw["sigma"]
                if isinstance(sigma, (tuple, list)) or not 0.0 < float(sigma) <= _lib.AUG_ELASTIC_MAX_RADIUS / 4.0:
                    raise NotImplementedError(f"ElasticTransformation: sigma={sigma!r} is not honoured (one number in (0, "
                                              f"{_lib.AUG_ELASTIC_MAX_RADIUS / 4.0}] for the whole pipeline)")
                self.elastic_sigma = float(sigma)
        self.base_seed = int(seed)
        self.seed = int(seed) + int(os.environ.get("LOCAL_RANK", "0"))
        self._rng = np.random.default_rng(self.seed)
        self._calls = 0
        self._salt_lut: dict = {}

    def __len__(self) -> int:
        return len(self.operators)

    def __repr__(self) -> str:
        return f"LabeledAugmentation({', '.join(f'{n}(p={p})' for n, p, _ in self.operators)})"

    # ------------------------------------------------------------------------------------------------ host: the draw
    def draw(self, b: int, h: int, w: int) -> dict:
        """one generator call per decision / parameter for the WHOLE batch (no Python loop over the images)"""
        r = self._rng
        table = np.zeros(b, dtype=ops.LABELAUG_DTYPE)
        table["image_id"] = np.arange(b)
        affine = np.tile(np.eye(3), (b, 1, 1))
        raw: dict[str, np.ndarray] = {}
        flags = np.zeros(b, dtype=np.int32)

        def note(key: str, on: np.ndarray, v) -> None:
            raw[key] = np.where(on, v, np.nan)

        for name, p, kw in self.operators:
            on = np.ones(b, dtype=bool) if p >= 1.0 else r.random(b) < p
            note(name, on, 1.0)
            if name == "Rot90":
                k = _sample_n(r, kw["k"], b, integer=True) % 4
                note("Rot90.k", on, k)
                turn = on & (k != 0)
                flags |= np.where(turn, _lib.AUG_GEOM, 0).astype(np.int32)
                quarter = np.stack([rot90_matrix(q, h, w) for q in range(4)])[k]
                affine = np.where(turn[:, None, None], quarter @ affine, affine)
            elif name == "Affine":
                rot, sc = _sample_n(r, kw["rotate"], b), _sample_n(r, kw["scale"], b)
                tp = kw["translate_percent"]
                tx, ty = (_sample_n(r, tp["x"], b), _sample_n(r, tp["y"], b)) if isinstance(tp, dict) else (_sample_n(r, tp, b), _sample_n(r, tp, b))
                note("Affine.rotate", on, rot), note("Affine.scale", on, sc), note("Affine.translate_x", on, tx), note("Affine.translate_y", on, ty)
                flags |= np.where(on, _lib.AUG_GEOM, 0).astype(np.int32)
                c, s_ = sc * np.cos(np.radians(rot)), sc * np.sin(np.radians(rot))   # scale, rotate (clockwise on the screen), translate
                m = np.tile(np.eye(3), (b, 1, 1))
                m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1] = c, -s_, s_, c
                m[:, 0, 2] = w / 2.0 + tx * w - (c * w / 2.0 - s_ * h / 2.0)
                m[:, 1, 2] = h / 2.0 + ty * h - (s_ * w / 2.0 + c * h / 2.0)
                affine = np.where(on[:, None, None], m @ affine, affine)
            elif name == "MotionBlur":
                k = _sample_n(r, kw["k"], b, integer=True)
                ang, d = _sample_n(r, kw["angle"], b), _sample_n(r, kw["direction"], b)
                note("MotionBlur.angle", on, ang), note("MotionBlur.direction", on, d)
                flags |= np.where(on, _lib.AUG_BLUR, 0).astype(np.int32)
                table["blur"][on] = motion_blur_weights_batch(k[on], ang[on], d[on]).reshape(-1, 25)
            elif name in ("CoarseDropout", "CoarseSalt", "CoarsePepper"):
                op = {"CoarseDropout": _lib.AUG_OP_DROPOUT, "CoarseSalt": _lib.AUG_OP_SALT, "CoarsePepper": _lib.AUG_OP_PEPPER}[name]
                prob, size = _sample_n(r, kw["p"], b), _sample_n(r, kw["size_percent"], b)
                note(f"{name}.p", on, prob), note(f"{name}.size_percent", on, size)
                flags |= np.where(on, {"CoarseDropout": _lib.AUG_DROPOUT, "CoarseSalt": _lib.AUG_SALT, "CoarsePepper": _lib.AUG_PEPPER}[name],
                                  0).astype(np.int32)
                table["coarse_gh"][:, op] = np.where(on, np.maximum(1, (h * size).astype(np.int64)), 0)
                table["coarse_gw"][:, op] = np.where(on, np.maximum(1, (w * size).astype(np.int64)), 0)
                table["coarse_thr"][:, op] = np.where(on, np.minimum((prob * (1 << 24)).astype(np.int64), 1 << 24), 0)
                if name == "CoarseDropout":
                    pc = kw["per_channel"]
                    per_channel = np.full(b, bool(pc)) if isinstance(pc, bool) else r.random(b) < float(pc)
                    note("CoarseDropout.per_channel", on, per_channel.astype(np.float64))
                    flags |= np.where(on & per_channel, _lib.AUG_DROP_PER_CHANNEL, 0).astype(np.int32)
            elif name == "ElasticTransformation":
                alpha = _sample_n(r, kw["alpha"], b)
                note("ElasticTransformation.alpha", on, alpha)
                flags |= np.where(on, _lib.AUG_ELASTIC, 0).astype(np.int32)
                table["elastic_alpha"] = np.where(on, alpha, 0.0)
            elif name == "AllChannelsHistogramEqualization":
                flags |= np.where(on, _lib.AUG_HISTEQ, 0).astype(np.int32)
            elif name == "AllChannelsCLAHE":
                clip, tiles = _sample_n(r, kw["clip_limit"], b), np.maximum(3, _sample_n(r, kw["tile_grid_size_px"], b, integer=True))
                note("AllChannelsCLAHE.clip_limit", on, clip), note("AllChannelsCLAHE.tile_grid_size_px", on, tiles)
                flags |= np.where(on, _lib.AUG_CLAHE, 0).astype(np.int32)
                ty, tx, count = clahe_geometry(h, w, tiles, clip)
                table["clahe_tiles_y"], table["clahe_tiles_x"], table["clahe_clip"] = np.where(on, ty, 0), np.where(on, tx, 0), np.where(on, count, 0)
                table["clahe_slot"] = np.where(on, np.cumsum(on) - 1, 0)
            elif name == "Emboss":
                alpha, strength = _sample_n(r, kw["alpha"], b), _sample_n(r, kw["strength"], b)
                note("Emboss.alpha", on, alpha), note("Emboss.strength", on, strength)
                flags |= np.where(on, _lib.AUG_EMBOSS, 0).astype(np.int32)
                table["emboss"][on] = emboss_weights(alpha[on], strength[on]).reshape(-1, 9)
            elif name == "CropAndPad":
                pct = np.stack([_sample_n(r, kw["percent"], b) for _ in range(4)], 1)  # top, right, bottom, left: independent (imgaug's default)
                for j, side in enumerate(("top", "right", "bottom", "left")):
                    note(f"CropAndPad.{side}", on, pct[:, j])
                px = np.rint(pct * np.array([h, w, h, w])).astype(np.int64)
                if ((h + px[:, 0] + px[:, 2] < 1) | (w + px[:, 1] + px[:, 3] < 1))[on].any():
                    raise ValueError(f"CropAndPad: percent {kw['percent']} removes a whole {h} x {w} image")
                flags |= np.where(on, _lib.AUG_CROPPAD, 0).astype(np.int32)
                table["pad"] = np.where(on[:, None], px, 0)
        table["flags"] = flags
        geom = (flags & _lib.AUG_GEOM) != 0
        if geom.any():
            table["geom"][geom] = np.linalg.inv(affine[geom])[:, :2].reshape(-1, 6)
        self._calls += 1
        return {"table": table, "affine": affine, "seed": (self.seed << 20) + self._calls, "raw": raw, "pipeline": self}

    # ------------------------------------------------------------------------------------------------ device: the stages before the resize
    def run(self, images_u8: torch.Tensor, drawn: dict, table_dev: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor | None]:
        """(B, H, W, 3) uint8 on the device -> (the images after every stage but crop-and-pad / resize, the elastic displacement field
        (B, 2, H, W) or None).  A fixed number of launches per batch, whatever its size."""
        table = drawn["table"]
        dev = images_u8.device
        b, h, w, _ = images_u8.shape
        if len(table) != b:
            raise ValueError(f"the drawn table has {len(table)} rows for a batch of {b}")
        t = ops.labelaug_table(table, dev) if table_dev is None else table_dev
        seed = int(drawn["seed"])
        x, field = images_u8, None
        flags = int(np.bitwise_or.reduce(table["flags"])) if b else 0
        for stage in self.stages:
            if stage == "geom" and flags & _lib.AUG_GEOM:
                x = ops.labelaug_geom(x, t)
            elif stage == "local" and flags & (_lib.AUG_BLUR | _lib.AUG_DROPOUT | _lib.AUG_SALT | _lib.AUG_PEPPER):
                if dev not in self._salt_lut:
                    self._salt_lut[dev] = torch.from_numpy(ops.salt_quantiles()).to(dev)
                x = ops.labelaug_local(x, t, _lib.AUG_LOCAL_BLUR_COARSE, seed, self._salt_lut[dev])
            elif stage == "elastic" and flags & _lib.AUG_ELASTIC:
                field = ops.labelaug_elastic_field(t, b, h, w, self.elastic_sigma, seed)
                x = ops.labelaug_elastic_apply(x, t, field)
            elif stage == "histeq" and flags & _lib.AUG_HISTEQ:
                x, _ = ops.labelaug_histeq(x, t)
            elif stage == "clahe" and flags & _lib.AUG_CLAHE:
                on = np.nonzero(table["flags"] & _lib.AUG_CLAHE)[0]
                order = on[np.argsort(table["clahe_slot"][on])]
                x = ops.labelaug_clahe(x, t, order.tolist(), int(table["clahe_tiles_y"][on].max()), int(table["clahe_tiles_x"][on].max()))
            elif stage == "emboss" and flags & _lib.AUG_EMBOSS:
                x = ops.labelaug_local(x, t, _lib.AUG_LOCAL_EMBOSS, seed)
        return x, field


def imgaug_transform(params_dict: dict, seed: int = 123456) -> LabeledAugmentation:
    """Parameter dictionary -> device pipeline.  Each key is an imgaug augmenter name, each value a dict with the optional keys "p"
    (probability, default 0.5; 0 drops the operator), "args" and "kwargs"; lists become tuples (two items) or the item (one item), as in the
    reference (yaml has no tuples; ``k: [[0, 2]]`` is the way to say "0 or 2")."""
    operators = []
    for name, spec in params_dict.items():
        name = str(name)
        if name not in _OPS:
            raise NotImplementedError(f"imgaug transform {name} is not implemented on the device (implemented: {list(_OPS)})")
        p = float(spec.get("p", 0.5))
        if spec.get("args", ()):
            raise NotImplementedError(f"{name}: positional args {list(spec['args'])} are not honoured, use kwargs")
        kwargs = {}
        for kw, arg in dict(spec.get("kwargs", {})).items():
            if hasattr(arg, "__len__") and not isinstance(arg, (str, dict, tuple)):  # list / ListConfig
                arg = list(arg)
                arg = arg[0] if len(arg) == 1 else (tuple(arg) if len(arg) == 2 else arg)
                if hasattr(arg, "__len__") and not isinstance(arg, (str, dict, tuple)):
                    arg = list(arg)
            if kw not in _OPS[name][2]:
                raise NotImplementedError(f"{name}: keyword {kw}={arg!r} is not honoured (honoured: {sorted(_OPS[name][2])})")
            kwargs[kw] = arg
        full = {**_DEFAULTS[name], **kwargs}
        if name == "Rot90" and full["keep_size"] is not True:
            raise NotImplementedError("Rot90: keyword keep_size=False is not honoured (the batch keeps one size)")
        if name == "CropAndPad" and (full["keep_size"] is not False or full["percent"] is None):
            raise NotImplementedError("CropAndPad: only percent=... with keep_size=False is honoured (keyword keep_size=True is not)")
        if name.startswith("Coarse") and full["size_percent"] is None:
            raise NotImplementedError(f"{name}: keyword size_percent is required (size_px is not honoured)")
        if name == "MotionBlur":
            ks = full["k"]
            ks = list(range(int(ks[0]), int(ks[1]) + 1)) if isinstance(ks, tuple) else (list(ks) if isinstance(ks, list) else [ks])
            if any(int(k) not in (3, 5) for k in ks):
                raise NotImplementedError(f"MotionBlur: keyword k={full['k']!r} is not honoured (3 or 5: the stencil has a 2-pixel halo)")
            full["k"] = [int(k) for k in ks]
        if name == "Affine" and isinstance(full["scale"], dict):
            raise NotImplementedError("Affine: keyword scale as a per-axis dict is not honoured")
        if name in ("CoarseSalt", "CoarsePepper") and full.get("per_channel"):
            raise NotImplementedError(f"{name}: keyword per_channel is not honoured")
        if p == 0.0:
            continue
        operators.append((name, p, full))
    return LabeledAugmentation(operators, seed=seed)


def get_imgaug_transform(cfg, seed: int = 123456) -> LabeledAugmentation:
    """``cfg.training.imgaug`` (preset string or parameter dictionary) -> pipeline (reference data/factory.py:47-100): multiview models with a
    camera-parameter file get "dlc-mv" (no per-view 2-D geometry) unless ``cfg.training.imgaug_3d`` is False."""
    def get(node, key, default=None):
        if isinstance(node, dict):
            return node.get(key, default)
        return node.get(key, default) if hasattr(node, "get") else getattr(node, key, default)

    training = get(cfg, "training")
    params = get(training, "imgaug", "default")
    if isinstance(params, str):
        imgaug_3d = get(training, "imgaug_3d", None)
        if (params not in ("default", "none") and str(get(get(cfg, "model"), "model_type", "")).find("multiview") > -1
                and get(get(cfg, "data"), "camera_params_file") and (imgaug_3d is True or imgaug_3d is None)):
            params = "dlc-mv"
        params_dict = expand_imgaug_str_to_dict(params)
    elif isinstance(params, dict) or type(params).__name__ == "DictConfig":
        if type(params).__name__ == "DictConfig":
            from omegaconf import OmegaConf

            params_dict = OmegaConf.to_object(params)
        else:
            params_dict = {k: dict(v) for k, v in params.items()}
    else:
        raise TypeError(f"params is of type {type(params)}, must be str, dict, or DictConfig")
    return imgaug_transform(params_dict, seed=seed)
