"""The flat-buffer layout of every executor, pinned: sizes, optimiser ranges, where each ``state_dict`` entry lives (buffer, offset,
shape, stride) and each layer's slot in the transposed copies - against tests/golden/engine_layout.json (this project's own offsets,
written by tests/golden/engine_layout.py).  A checkpoint, the optimiser's ranges and the gradient buckets all depend on them.  Also the
class structure: the ViT and head executors share the core with the ResNet executor, not its BatchNorm code."""

import json
import os

import pytest

from tests.conftest import GOLDEN
from tests.golden.engine_layout import build_cases, describe

CASES = ("resnet", "vit", "vit_views2", "vit_dinov2", "head", "head_options")


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "engine_layout.json")) as f:
        return json.load(f)


def test_layout_matches_golden(stack_backend, want):
    engines = build_cases(stack_backend)
    assert tuple(engines) == CASES and sorted(want) == sorted(CASES)
    for name, eng in engines.items():
        got = json.loads(json.dumps(describe(eng)))   # (tuples -> lists, as the file holds them)
        for field in ("n_total", "n_wd", "n_running", "group_ranges", "wd_off"):
            assert got[field] == want[name][field], (name, field)
        assert list(got["state_dict"]) == list(want[name]["state_dict"]), name   # (same keys in the same order)
        for k, v in got["state_dict"].items():
            assert v == want[name]["state_dict"][k], (name, k)


def test_vit_and_head_executors_are_not_resnet_executors():
    from lightning_pose_amd.engine import Engine, HeadEngine
    from lightning_pose_amd.vit_engine import ViTEngine

    assert not issubclass(ViTEngine, Engine)
    assert not issubclass(HeadEngine, Engine)
    assert not hasattr(ViTEngine, "_bn_fwd")
