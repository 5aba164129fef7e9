"""The SAM tracker's step configuration, registered next to tests/golden/step_inputs.py's (which is not edited): importing this module adds
STEP_CONFIGS["sam"], so that ``make_step_inputs("sam", ...)`` and ``seeded_backbone_weights`` serve it like the others.

width 128 / 3 layers (layer 1 global) / 2 heads / MLP 256, window 4 on 96-px frames: a 6 x 6 token grid padded to 8 x 8 - four windows, three
of them ragged, 28 of the 64 window rows padding.  K = 3 keypoints, 4 labeled + 6 unlabeled frames, heatmap_mse + temporal + pca_singleview.
The HF module is built with a 128-px pretraining image (8 x 8 position table, resized to 6 x 6 by the reference's wrapper) and 32 neck
channels."""

from tests.golden.step_inputs import STEP_CONFIGS

# hidden, depth, heads, mlp, patch, window, global layers, pretraining grid, neck channels: SAM_CONFIGS["vitb_sam"] for this configuration
SAM_VIT = (128, 3, 2, 256, 16, 4, (1,), 8, 32)
STEP_CONFIGS.setdefault("sam", dict(HW=96, K=3, Bl=4, S=6, V=1, seed=33, unsup=("temporal", "pca_singleview"), backbone="vitb_sam"))
