from .factory import BACKBONE_STRIDES, backbone_features, tracker_backbone_features  # noqa: F401
