"""The multi-view transformer's step configuration, registered next to tests/golden/step_inputs.py's (which is not edited): importing this
module adds STEP_CONFIGS["mvt"], so that ``make_step_inputs("mvt", ...)`` and ``seeded_backbone_weights`` serve it like the others.

width 128 / 2 layers / 2 heads / MLP 256, 3 x 3 pretraining grid (the emulator-sized ViT of tests/test_emu_vit_engine.py), 64-px views,
V = 3 views, K = 3 keypoints, 2 labeled + 3 unlabeled samples, heatmap_mse + temporal + pca_multiview."""

from tests.golden.step_inputs import STEP_CONFIGS

MVT_VIT = (128, 2, 2, 256, 16, 3)    # hidden, depth, heads, mlp, patch, pretraining grid: VIT_CONFIGS["vits_dino"] for this configuration
STEP_CONFIGS.setdefault("mvt", dict(HW=64, K=3, Bl=2, S=3, V=3, seed=31, unsup=("temporal", "pca_multiview"), backbone="vits_dino"))
