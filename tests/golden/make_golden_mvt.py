"""Generate tests/golden/step_mvt.npz: one semi-supervised training step of the reference's OWN
SemiSupervisedHeatmapTrackerMultiviewTransformer (verbatim module under oracle/ref_loader.py's stubs, fp32, torch CPU) on the seeded inputs
of tests/golden/step_inputs_mvt.py.  Build container only (needs the reference tree):

    python tests/golden/make_golden_mvt.py

The file holds arrays and name lists only - the trained head and the view embeddings both sides start from, every logged scalar, the total
loss, what the losses saw (heat-maps, keypoints, confidences) and the parameter gradients (the head's, the embeddings', every LayerNorm's and
bias in full; one norm per parameter tensor) - in the layout of make_golden.py::gen_step_parity, so tests/test_step_parity.py's checker reads it.
"""

from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import transformers  # noqa: E402  (before any stub is installed, as in make_golden.py)

from oracle import ref_loader as R  # noqa: E402
from tests.golden.make_golden import save  # noqa: E402
from tests.golden.step_inputs import (HEAD_TRAIN_LR, HEAD_TRAIN_STEPS, PCA_LOG_WEIGHT, TEMPORAL, TORCH_SEED, make_step_inputs,  # noqa: E402
                                      seeded_backbone_weights)
from tests.golden.step_inputs_mvt import MVT_VIT  # noqa: E402  (registers STEP_CONFIGS["mvt"])

VIEW_SEED, VIEW_STD = 41, 0.5    # view embeddings both sides load (0.02, the initialisation, would leave the views almost without effect)


def view_embeddings(V: int, D: int) -> torch.Tensor:
    return VIEW_STD * torch.randn(V, D, generator=torch.Generator().manual_seed(VIEW_SEED))


def load_verbatim_module():
    """the reference's models/heatmap_tracker_multiview.py; its calibration imports get a stand-in module, its ViT comes from a config"""
    R.install_stubs()
    cameras = types.ModuleType("lightning_pose.data.cameras")

    def _no_calibration(*a, **k):
        raise NotImplementedError("no camera calibration in this fixture")
    cameras.project_3d_to_2d = cameras.project_camera_pairs_to_3d = _no_calibration
    sys.modules["lightning_pose.data.cameras"] = cameras
    hidden, depth, heads, mlp, patch, grid = MVT_VIT

    def _from_config(model_name, add_pooling_layer=False, **kw):
        c = transformers.ViTConfig(hidden_size=hidden, num_hidden_layers=depth, num_attention_heads=heads, intermediate_size=mlp,
                                   patch_size=patch, image_size=patch * grid, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        return transformers.ViTModel(c, add_pooling_layer=add_pooling_layer)
    transformers.ViTModel.from_pretrained = staticmethod(_from_config)
    return R.load("models.heatmap_tracker_multiview")


def _train_head(model, inp, gen_hm, steps, lr):
    """make_golden.py::_train_head for this model: Adam on the head alone over the cached transformer features of the step's own views"""
    cfg, batch = inp["cfg"], inp["batch"]
    K, HW = cfg["K"], cfg["HW"]
    h = HW // 4
    sets = [(batch["labeled"]["images"].reshape(-1, 3, HW, HW), batch["labeled"]["heatmaps"].reshape(-1, K, h, h)),
            (batch["unlabeled"]["frames"].reshape(-1, 3, HW, HW), gen_hm(inp["unl_centres"].clone(), HW, HW, (h, h)))]
    model.train()
    with torch.no_grad():
        feats = [(model.forward_vit(x), t) for x, t in sets]
    opt = torch.optim.Adam(model.head.parameters(), lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        loss = 0.0
        for f, t in feats:
            p = model.head(f)
            keep = t.flatten(2).sum(-1) > 0
            loss = loss + ((p - t) ** 2)[keep].mean() * h * h
        loss.backward()
        opt.step()
    model.zero_grad()
    return float(loss)


def gen_step_mvt():
    M = load_verbatim_module()
    Fa, L, H = R.load("losses.factory"), R.load("losses.losses"), R.load("data.heatmaps")
    inp = make_step_inputs("mvt", H.generate_heatmaps)
    cfg, batch = inp["cfg"], inp["batch"]
    K, V, HW = cfg["K"], cfg["V"], cfg["HW"]
    sup = Fa.LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None)
    unsup = Fa.LossFactory({"temporal": dict(TEMPORAL)}, None)
    kpca = R.fit_keypoint_pca("pca_multiview", inp["pca_fit"], components_to_keep=3, mirrored_column_matches=inp["mcm"],
                              columns_for_singleview_pca=None)
    loss = L.PCALoss.__new__(L.PCALoss)
    L.Loss.__init__(loss, log_weight=PCA_LOG_WEIGHT)
    loss.device, loss.loss_name, loss.pca = "cpu", "pca_multiview", kpca
    loss.epsilon = kpca.parameters["epsilon"]
    unsup.loss_instance_dict["pca_multiview"] = loss
    model = M.SemiSupervisedHeatmapTrackerMultiviewTransformer(num_keypoints=K, num_views=V, loss_factory=sup, loss_factory_unsupervised=unsup,
                                                               backbone="vits_dino", pretrained=False, torch_seed=TORCH_SEED, image_size=HW)
    model.total_unsupervised_importance = torch.tensor(1.0)
    sd = model.state_dict()
    assert list(sd)[0] == "view_embeddings" and [g["name"] for g in model.get_parameters()] == ["backbone", "head", "view_embeddings"]
    new = seeded_backbone_weights(sd)
    sd.update(new)
    sd["view_embeddings"] = view_embeddings(V, MVT_VIT[0])
    model.load_state_dict(sd)
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
    arrs["backbone_names"] = np.array(sorted(new))
    arrs["state_dict_names"] = np.array(list(sd))
    out = model.training_step(batch, 0)
    out["loss"].backward()
    logged = {k: float(v) for k, v in model.logged.items()}
    arrs.update(log_names=np.array(list(logged)), log_values=np.array(list(logged.values())), loss=out["loss"].detach(),
                head_fit_loss=np.float32(fit_loss))
    assert {k for k, v in seen["get_loss_inputs_labeled"].items() if v is None} == {"keypoints_targ_3d", "keypoints_pred_3d",
                                                                                   "keypoints_pred_2d_reprojected"}
    for meth, tag in (("get_loss_inputs_labeled", "lab"), ("get_loss_inputs_unlabeled", "unl")):
        d = seen[meth]
        for k in ("keypoints_pred", "keypoints_pred_augmented", "confidences", "keypoints_targ"):
            if k in d:
                arrs[f"{tag}_{k}"] = d[k]
        hm = d["heatmaps_pred"]
        flat = hm.reshape(hm.shape[0], hm.shape[1], -1)
        arrs[f"{tag}_heat_max"], arrs[f"{tag}_heat_argmax"], arrs[f"{tag}_heat"] = flat.max(-1).values, flat.argmax(-1), hm
    arrs.update(pca_mean=kpca.parameters["mean"], pca_kept=kpca.parameters["kept_eigenvectors"], pca_eps=kpca.parameters["epsilon"])
    grads = {n_: (p_.grad if p_.grad is not None else torch.zeros_like(p_)) for n_, p_ in model.named_parameters()}
    for n_, gr in grads.items():   # in full: the head, the embeddings, every one-dimensional tensor (LayerNorms, biases); a norm for all
        if n_.startswith("head.") or n_ == "view_embeddings" or ".embeddings." in n_ and gr.numel() <= 4096 or gr.dim() == 1:
            arrs["grad/" + n_] = gr
    names_sorted = sorted(grads)
    arrs["grad_names"] = np.array(names_sorted)
    arrs["grad_norms"] = np.array([float(grads[n_].norm()) for n_ in names_sorted])
    save("step_mvt", **arrs)
    print("   ", {k: round(v, 6) for k, v in logged.items()}, "head fit", round(fit_loss, 6))


if __name__ == "__main__":
    torch.set_num_threads(8)
    gen_step_mvt()
