"""Twin of drone/models/cfp/yolox_cfp.py (the "centralized feature pyramid"): `YoloBody(num_classes, phi)`, the plain YOLOX
with an EVCBlock on the upsampled P5 lateral of the top-down path, HIP backed."""
from glsdet_amd.drone.body import CfpYoloBody as YoloBody  # noqa: F401
