# Coarse detector of UFPMP-Det on a Swin-T backbone (backbones/swin.py:466-640): GFL = SwinTransformer + FPN + GFLHead.
# The trunk hands stages 1..3 (strides 8 / 16 / 32, widths 192 / 384 / 768) to the FPN, which therefore starts at level 0;
# head and test settings are coarse_det.py's.
_base_ = ['./coarse_det.py']
model = dict(
    backbone=dict(
        _delete_=True,
        type='SwinTransformer', embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, mlp_ratio=4,
        qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2, patch_norm=True,
        out_indices=(1, 2, 3), with_cp=False),
    neck=dict(in_channels=[192, 384, 768], start_level=0))
