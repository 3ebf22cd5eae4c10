"""strolle_amd — MI355X-native hot path of Patryk27/strolle (BVH traversal, ReSTIR DI/GI, SVGF).

The product is the C-ABI shared library `strolle_amd/csrc/libstrolle_hip.so`
(include/strolle_hip.h); this package is its Python host-side mirror of
`strolle::Engine` plus scene helpers for the benchmark scenes.
"""
from .api import (LENS_FIT, LENS_VIGNETTE_ROUND, LENS_GRAIN_ANIMATE, StLensDesc, StLensPlan, lens_desc, lens_plan, GRADE_DITHER, LutDomain, StColorGradingDesc, StColorGradingPlan, color_grading_desc, color_grading_plan, decode_cube, load_cube, Aov, Buffer, Camera, OutputFormat, CameraMode, Engine, FogFalloff, FOG_SKY, FOG_FOLLOW_SUN, StFogDesc, fog_desc, StLightShaftsDesc, light_shafts_desc, light_shafts_plan, SHAFTS_FOLLOW_SUN, SHAFTS_LIGHT_EXTINCTION, Instance, Light, Material, Mesh, PassBit, ResampleFilter, StrolleError, Sun, Tonemap,  # noqa: F401
                  MORPH_DELTA_DTYPE, SKIN_VERTEX_DTYPE, StMorphDelta, StSkinVertex, aov_planes, bloom_desc, motion_blur_desc, dof_desc, dof_plan, decode_hdr, display_desc, load_hdr, post_desc, upscale_desc, StUpscaleDesc, UPSCALE_DENOISE, look_at_transform, perspective_infinite_reverse_rh)
