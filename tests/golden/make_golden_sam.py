"""Generate tests/golden/step_sam.npz: one semi-supervised training step of the reference's OWN SemiSupervisedHeatmapTracker with
``backbone="vitb_sam"`` (verbatim modules under oracle/ref_loader.py's stubs - models/heatmap_tracker.py, models/backbones/factory.py and
vit_sam.py - fp32, torch CPU) on the seeded inputs of tests/golden/step_inputs_sam.py.  Build container only (needs the reference tree):

    python tests/golden/make_golden_sam.py

``SamModel.from_pretrained`` cannot download anything here, so it is replaced by a constructor of the same architecture from a small config
(step_inputs_sam.SAM_VIT), the way make_golden_mvt.py replaces ``ViTModel.from_pretrained``; everything after it - the wrapper's position-table
resize to the fine-tuning grid, ``use_rel_pos = False``, the neck-free forward - is the reference's own code.  The file holds arrays and name
lists only, in the layout of make_golden.py::gen_step_parity, so tests/test_step_parity.py's checker reads it.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import transformers  # noqa: E402  (before any stub is installed, as in make_golden.py)

from oracle import ref_loader as R  # noqa: E402
from tests.golden.make_golden import _train_head, save  # noqa: E402
from tests.golden.step_inputs import (HEAD_TRAIN_LR, HEAD_TRAIN_STEPS, PCA_LOG_WEIGHT, TEMPORAL, TORCH_SEED, make_step_inputs,  # noqa: E402
                                      seeded_backbone_weights)
from tests.golden.step_inputs_sam import SAM_VIT  # noqa: E402  (registers STEP_CONFIGS["sam"])


def small_sam_model(model_name="facebook/sam-vit-base", **kw):
    """what stands in for ``SamModel.from_pretrained``: a ``SamModel`` of step_inputs_sam.SAM_VIT's vision config"""
    assert model_name == "facebook/sam-vit-base", model_name
    hidden, depth, heads, mlp, patch, window, global_layers, grid0, neck = SAM_VIT
    vision = transformers.SamVisionConfig(hidden_size=hidden, num_hidden_layers=depth, num_attention_heads=heads, mlp_dim=mlp, patch_size=patch,
                                          image_size=patch * grid0, window_size=window, global_attn_indexes=list(global_layers),
                                          output_channels=neck)
    return transformers.SamModel(transformers.SamConfig(vision_config=vision))


def load_verbatim_module():
    R.install_stubs()
    transformers.SamModel.from_pretrained = staticmethod(small_sam_model)
    return R.load("models.heatmap_tracker")


def build_reference_tracker(inp):
    """the reference's tracker for the step's configuration, its backbone overwritten with the seeded draw both sides share; also returns
    the names of the tensors that draw covers and the fitted PCA"""
    T = load_verbatim_module()
    Fa, L = R.load("losses.factory"), R.load("losses.losses")
    cfg = inp["cfg"]
    sup = Fa.LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None)
    unsup = Fa.LossFactory({"temporal": dict(TEMPORAL)}, None)
    kpca = R.fit_keypoint_pca("pca_singleview", inp["pca_fit"], components_to_keep=0.99, mirrored_column_matches=inp["mcm"],
                              columns_for_singleview_pca=inp["cols"])
    loss = L.PCALoss.__new__(L.PCALoss)
    L.Loss.__init__(loss, log_weight=PCA_LOG_WEIGHT)
    loss.device, loss.loss_name, loss.pca = "cpu", "pca_singleview", kpca
    loss.epsilon = kpca.parameters["epsilon"]
    unsup.loss_instance_dict["pca_singleview"] = loss
    model = T.SemiSupervisedHeatmapTracker(num_keypoints=cfg["K"], loss_factory=sup, loss_factory_unsupervised=unsup, backbone="vitb_sam",
                                           pretrained=False, torch_seed=TORCH_SEED, image_size=cfg["HW"])
    model.total_unsupervised_importance = torch.tensor(1.0)
    sd = model.state_dict()
    grid = cfg["HW"] // SAM_VIT[4]
    assert sd["backbone.vision_encoder.pos_embed"].shape == (1, grid, grid, SAM_VIT[0])      # resized by the wrapper, at construction
    new = seeded_backbone_weights(sd)
    sd.update(new)
    model.load_state_dict(sd)
    return model, sorted(new), list(sd), kpca


def gen_step_sam():
    H = (R.install_stubs(), R.load("data.heatmaps"))[1]
    inp = make_step_inputs("sam", H.generate_heatmaps)
    batch = inp["batch"]
    model, backbone_names, sd_names, kpca = build_reference_tracker(inp)
    fit_loss = _train_head(model, inp, H.generate_heatmaps, HEAD_TRAIN_STEPS, HEAD_TRAIN_LR)
    seen = {}
    for meth in ("get_loss_inputs_labeled", "get_loss_inputs_unlabeled"):
        orig = getattr(model, meth)

        def wrapped(batch_dict, _orig=orig, _m=meth):
            d = _orig(batch_dict)
            seen[_m] = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in d.items()}
            return d
        setattr(model, meth, wrapped)
    model.train()
    arrs = {"head/" + n_: p_.detach().clone() for n_, p_ in model.head.named_parameters()}
    arrs["backbone_names"] = np.array(backbone_names)
    arrs["state_dict_names"] = np.array(sd_names)
    out = model.training_step(batch, 0)
    out["loss"].backward()
    logged = {k: float(v) for k, v in model.logged.items()}
    arrs.update(log_names=np.array(list(logged)), log_values=np.array(list(logged.values())), loss=out["loss"].detach(),
                head_fit_loss=np.float32(fit_loss))
    for meth, tag in (("get_loss_inputs_labeled", "lab"), ("get_loss_inputs_unlabeled", "unl")):
        d = seen[meth]
        for k in ("keypoints_pred", "keypoints_pred_augmented", "confidences", "keypoints_targ"):
            if k in d:
                arrs[f"{tag}_{k}"] = d[k]
        hm = d["heatmaps_pred"]
        flat = hm.reshape(hm.shape[0], hm.shape[1], -1)
        arrs[f"{tag}_heat_max"], arrs[f"{tag}_heat_argmax"], arrs[f"{tag}_heat"] = flat.max(-1).values, flat.argmax(-1), hm
    arrs.update(pca_mean=kpca.parameters["mean"], pca_kept=kpca.parameters["kept_eigenvectors"], pca_eps=kpca.parameters["epsilon"])
    # the tensors the forward pass reads have a gradient; rel_pos_* and neck.* have none (grad is None) and are listed apart
    grads = {n_: p_.grad for n_, p_ in model.named_parameters() if p_.grad is not None}
    arrs["no_grad_names"] = np.array(sorted(n_ for n_, p_ in model.named_parameters() if p_.grad is None))
    for n_, gr in grads.items():   # in full: the head, the position table, every one-dimensional tensor (LayerNorms, biases); a norm for all
        if n_.startswith("head.") or n_.endswith("pos_embed") or gr.dim() == 1:
            arrs["grad/" + n_] = gr
    names_sorted = sorted(grads)
    arrs["grad_names"] = np.array(names_sorted)
    arrs["grad_norms"] = np.array([float(grads[n_].norm()) for n_ in names_sorted])
    save("step_sam", **arrs)
    print("   ", {k: round(v, 6) for k, v in logged.items()}, "head fit", round(fit_loss, 6))


if __name__ == "__main__":
    torch.set_num_threads(8)
    gen_step_sam()
