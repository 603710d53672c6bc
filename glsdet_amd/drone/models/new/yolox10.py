"""Twin of drone/models/new/yolox10.py (named next to yolox6 as a final model, get_map.py): `YoloBody(num_classes, phi)`
with the residual Patch_Conv_NonLocal_new blocks on dark3 / dark4 / dark5 and the cross-scale decoupled head, HIP backed."""
from glsdet_amd.drone.body import Cross10YoloBody as YoloBody  # noqa: F401
