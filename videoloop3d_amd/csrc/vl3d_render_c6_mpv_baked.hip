// MPV.py:351-454 planar convention (affine texel transform, hard-cut quad borders) under the bake rule (VL3D_ACT_BAKED, include/vl3d.h):
// every tap activated, truncated to the byte the viewer package ships, decoded and then blended -- the picture a player shows, trained
// with the activate-first gradient (the rounding straight-through).  Shipped activations, fp32 and fp16 stacks
#define VL3D_CONV_FN conv_affine_hardcut_baked
#define VL3D_CONV_COORD VL3D_COORD_AFFINE
#define VL3D_CONV_BORDER VL3D_BORDER_HARDCUT
#define VL3D_CONV_ORDER VL3D_ACT_BAKED
#define VL3D_CONV_ACTS 0
#include "vl3d_render_conv.inc"
