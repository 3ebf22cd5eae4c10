"""Python host-side mirror of `strolle::Engine` over the C ABI of libstrolle_hip.so.

Names, argument meaning and error behaviour follow the reference's public API
(strolle/src/lib.rs:105-409, camera.rs, light.rs, material.rs, instance.rs,
mesh_triangle.rs, sun.rs) so tests read like reference usage. This module is a
thin ctypes binding: all engine logic (scene stores, BVH build, pass graph) is
C++ inside the shared library, all per-pixel work is HIP. There is no CPU
fallback: if the library or a GPU is missing, calls raise.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import enum
import math
import os
import sys
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STROLLE_HIP_LIB") or os.path.join(_HERE, "csrc", "libstrolle_hip.so")   # STROLLE_HIP_LIB: another build of the library (same-box A/B of two builds)
if os.environ.get("STROLLE_HIP_LIB"):  # experiments: an alternative build of the same sources (never a different implementation)
    LIB_PATH = os.environ["STROLLE_HIP_LIB"]


# ----------------------------------------------------------------------------- C structs (include/strolle_hip.h)
class StMeshTriangle(C.Structure):
    _fields_ = [("positions", C.c_float * 9), ("normals", C.c_float * 9), ("uvs", C.c_float * 6), ("tangents", C.c_float * 12)]


class StSkinVertex(C.Structure):
    """include/strolle_hip.h "skinned meshes": one corner's joint indices and weights (24 B)."""
    _fields_ = [("joints", C.c_uint16 * 4), ("weights", C.c_float * 4)]


SKIN_VERTEX_DTYPE = np.dtype({"names": ["joints", "weights"], "formats": [(np.uint16, (4,)), (np.float32, (4,))], "offsets": [0, 8], "itemsize": 24})


class StMorphDelta(C.Structure):
    """include/strolle_hip.h "morph targets": one corner's displacement under one target (24 B)."""
    _fields_ = [("position", C.c_float * 3), ("normal", C.c_float * 3)]


MORPH_DELTA_DTYPE = np.dtype({"names": ["position", "normal"], "formats": [(np.float32, (3,)), (np.float32, (3,))], "offsets": [0, 12], "itemsize": 24})


class StMaterial(C.Structure):
    _fields_ = [
        ("base_color", C.c_float * 4), ("emissive", C.c_float * 4),
        ("perceptual_roughness", C.c_float), ("metallic", C.c_float), ("reflectance", C.c_float), ("ior", C.c_float),
        ("base_color_texture", C.c_uint64), ("emissive_texture", C.c_uint64),
        ("metallic_roughness_texture", C.c_uint64), ("normal_map_texture", C.c_uint64),
        ("alpha_mode", C.c_uint32), ("_pad", C.c_uint32),
    ]


class StLight(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("position", C.c_float * 3), ("radius", C.c_float), ("color", C.c_float * 3),
                ("range", C.c_float), ("direction", C.c_float * 3), ("angle", C.c_float)]


class StCamera(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("denoise", C.c_uint32), ("depth", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("pos_x", C.c_uint32), ("pos_y", C.c_uint32), ("_pad", C.c_uint32), ("transform", C.c_float * 16), ("projection", C.c_float * 16)]


class StDistRect(C.Structure):
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32)]

    def as_tuple(self):
        return (self.x0, self.y0, self.x1, self.y1)


class StDistGrid(C.Structure):
    """include/strolle_hip.h StDistGrid: a (cost-weighted) tile grid every rank holds identically."""
    _fields_ = [("cols", C.c_uint32), ("rows", C.c_uint32), ("row_edge", C.c_uint32 * 17), ("col_edge", (C.c_uint32 * 17) * 16)]

    def tiles(self):
        return [dist_grid_tile(self, r) for r in range(self.cols * self.rows)]

    def describe(self):
        return {"cols": self.cols, "rows": self.rows, "row_edges": list(self.row_edge[:self.rows + 1]),
                "col_edges": [list(self.col_edge[k][:self.cols + 1]) for k in range(self.rows)]}


class StDistUniqueId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]


class StTuning(C.Structure):
    """include/strolle_hip.h StTuning: scheduling / tuning switches of one engine."""
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "overlap", "fuse", "fuse_di_head", "fuse_spatial", "fuse_gi_sampling", "fuse_gi_validation",
                                          "fuse_gi_reprojection", "fuse_wavelet", "fuse_compose", "preview_both", "variance_in_reproject",
                                          "lean_frame", "skip_scratch_stores", "di_head_on_main", "alias_gi_history", "tile_map", "tile_map_denoise")] + \
               [("side_priority", C.c_int32)] + \
               [(n, C.c_uint32) for n in ("staging", "double_buffer", "packed_base", "tick_timing", "anyhit_fast", "compact_bvh",
                                          "allow_deep_bvh", "device_bake", "wide_bvh", "wide_stack_entries", "primary_packets", "side_start")]


PROFILE_MAX_KERNELS = 64   # ST_PROFILE_MAX_KERNELS


class StKernelProfile(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint32), ("total_ms", C.c_float), ("algorithmic_bytes", C.c_double), ("traversal_bytes", C.c_double)]


class StGltfOptions(C.Structure):
    _fields_ = [("first_handle", C.c_uint64), ("first_image_handle", C.c_uint64), ("override_mask", C.c_uint32), ("reflectance", C.c_float),
                ("perceptual_roughness", C.c_float), ("subdivide", C.c_uint32), ("light_radius", C.c_float), ("_pad", C.c_uint32)]


class StGltfSummary(C.Structure):
    _fields_ = [("meshes", C.c_uint32), ("triangles", C.c_uint32), ("materials", C.c_uint32), ("images", C.c_uint32), ("images_dropped", C.c_uint32),
                ("primitives_skipped", C.c_uint32), ("lights", C.c_uint32), ("lights_skipped", C.c_uint32)]


assert C.sizeof(StMeshTriangle) == 144 and C.sizeof(StMaterial) == 88 and C.sizeof(StLight) == 52 and C.sizeof(StCamera) == 160


class StEnvironmentDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("intensity", C.c_float), ("yaw", C.c_float)]


ENV_KEEP_SUN, ENV_UNIFORM_SAMPLING = 1, 2
ENV_CELL_DTYPE = np.dtype([("q", np.float32), ("alias", np.uint32), ("p", np.float32)])   # one cell of the importance table (12 B)


def environment_desc(intensity: float = 1.0, yaw: float = 0.0, keep_sun: bool = False, uniform: bool = False) -> StEnvironmentDesc:
    return StEnvironmentDesc(C.sizeof(StEnvironmentDesc), (ENV_KEEP_SUN if keep_sun else 0) | (ENV_UNIFORM_SAMPLING if uniform else 0),
                             float(intensity), float(yaw))


class Tonemap(enum.IntEnum):
    """include/strolle_hip.h StTonemap: the operator of a camera's display transform"""
    NONE = 0
    REINHARD = 1
    REINHARD_LUMINANCE = 2
    ACES_FITTED = 3
    PBR_NEUTRAL = 4


class StDisplayDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tonemap", C.c_uint32), ("flags", C.c_uint32), ("exposure_ev", C.c_float),
                ("ev_min", C.c_float), ("ev_max", C.c_float), ("low_fraction", C.c_float), ("high_fraction", C.c_float),
                ("max_ev_step_up", C.c_float), ("max_ev_step_down", C.c_float)]


DISPLAY_AUTO_EXPOSURE = 1
DISPLAY_BINS = 64


def display_desc(tonemap=Tonemap.NONE, exposure_ev: float = 0.0, auto_exposure: bool = False, ev_min: float = -8.0, ev_max: float = 8.0,
                 low_fraction: float = 0.1, high_fraction: float = 0.9, max_ev_step_up: float = 0.0, max_ev_step_down: float = 0.0) -> StDisplayDesc:
    """A StDisplayDesc. Manual: scale = 2^exposure_ev. auto_exposure: exposure_ev is the compensation, the rest meters and adapts
    (include/strolle_hip.h "display transforms")."""
    return StDisplayDesc(C.sizeof(StDisplayDesc), int(tonemap), DISPLAY_AUTO_EXPOSURE if auto_exposure else 0, float(exposure_ev),
                         float(ev_min), float(ev_max), float(low_fraction), float(high_fraction), float(max_ev_step_up), float(max_ev_step_down))


class ResampleFilter(enum.IntEnum):
    """include/strolle_hip.h StResampleFilter: how post-processing resamples the frame to the output size"""
    NEAREST = 0
    BILINEAR = 1
    CATMULL_ROM = 2


class StPostDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("output_width", C.c_uint32), ("output_height", C.c_uint32),
                ("filter", C.c_uint32), ("fxaa_edge_threshold", C.c_float), ("fxaa_edge_threshold_min", C.c_float), ("fxaa_subpixel", C.c_float)]


POST_FXAA = 1


def post_desc(fxaa: bool = False, output_size=None, filter=ResampleFilter.BILINEAR, fxaa_edge_threshold: float = 0.0,
              fxaa_edge_threshold_min: float = 0.0, fxaa_subpixel: float = 0.75) -> StPostDesc:
    """A StPostDesc: FXAA on the display-referred colour and / or resampling to output_size = (width, height) (None: the render size);
    thresholds of 0 are FXAA 3.11's defaults (include/strolle_hip.h "post-processing")."""
    ow, oh = output_size if output_size else (0, 0)
    return StPostDesc(C.sizeof(StPostDesc), POST_FXAA if fxaa else 0, int(ow), int(oh), int(filter), float(fxaa_edge_threshold),
                      float(fxaa_edge_threshold_min), float(fxaa_subpixel))


class StUpscaleDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("output_width", C.c_uint32), ("output_height", C.c_uint32),
                ("sharpness", C.c_float), ("_pad", C.c_uint32 * 3)]


UPSCALE_DENOISE = 1


def upscale_desc(output_size=None, sharpness: float = 0.0, denoise: bool = False) -> StUpscaleDesc:
    """A StUpscaleDesc: the edge-adaptive upscaler to output_size = (width, height) (None: the render size, sharpen only) and / or the
    contrast-adaptive sharpening step at `sharpness` in 0..1 (0: none), `denoise`: its noise limiter (include/strolle_hip.h "upscaling")."""
    ow, oh = output_size if output_size else (0, 0)
    return StUpscaleDesc(C.sizeof(StUpscaleDesc), UPSCALE_DENOISE if denoise else 0, int(ow), int(oh), float(sharpness))


class StMotionBlurDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("samples", C.c_uint32), ("shutter", C.c_float), ("max_radius", C.c_float),
                ("depth_softness", C.c_float)]


MOTION_BLUR_NO_JITTER = 1


def motion_blur_desc(shutter: float = 0.5, samples: int = 0, max_radius: float = 0.0, depth_softness: float = 0.0, jitter: bool = True) -> StMotionBlurDesc:
    """A StMotionBlurDesc; the defaults are Bevy's shutter angle of 0.5, 8 samples, a 32-pixel radius and a depth softness of 0.05
    (include/strolle_hip.h "motion blur")."""
    return StMotionBlurDesc(C.sizeof(StMotionBlurDesc), 0 if jitter else MOTION_BLUR_NO_JITTER, int(samples), float(shutter), float(max_radius),
                            float(depth_softness))


class StDofDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("samples", C.c_uint32), ("focal_distance", C.c_float), ("aperture_f_stops", C.c_float),
                ("sensor_height", C.c_float), ("max_radius", C.c_float), ("focus_x", C.c_float), ("focus_y", C.c_float), ("_pad", C.c_uint32)]


DOF_AUTOFOCUS, DOF_PLANAR_DEPTH, DOF_MAX_SAMPLES = 1, 2, 64


def dof_desc(focal_distance: float = 10.0, aperture_f_stops: float = 0.0, sensor_height: float = 0.0, samples: int = 0, max_radius: float = 0.0,
             autofocus=None, planar_depth: bool = False) -> StDofDesc:
    """A StDofDesc; the defaults are Bevy's focal distance of 10 m, f/1, a Super 35 sensor (18.66 mm), 32 samples and a 32-pixel radius
    (include/strolle_hip.h "depth of field"). autofocus: None, or the focus point (x, y) in [0, 1]^2 of the frame."""
    fx, fy = (float(autofocus[0]), float(autofocus[1])) if autofocus is not None else (0.0, 0.0)
    return StDofDesc(C.sizeof(StDofDesc), (DOF_AUTOFOCUS if autofocus is not None else 0) | (DOF_PLANAR_DEPTH if planar_depth else 0), int(samples), float(focal_distance),
                     float(aperture_f_stops), float(sensor_height), float(max_radius), fx, fy, 0)


def dof_plan(desc: StDofDesc, width: int, height: int):
    """st_dof_plan (pure host): (samples, (tiles_x, tiles_y), the tap table as a (samples, 3) float32 array of (x, y, rho))."""
    import numpy as np
    lib = load_library()
    lib.st_dof_plan.restype = C.c_int
    lib.st_dof_plan.argtypes = [C.POINTER(StDofDesc), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    n, tiles, taps = C.c_uint32(), (C.c_uint32 * 2)(), (C.c_float * (DOF_MAX_SAMPLES * 3))()
    rc = lib.st_dof_plan(C.byref(desc), width, height, C.byref(n), tiles, taps)
    if rc != 0:
        lib.st_last_error.restype = C.c_char_p
        raise StrolleError(f"{_STATUS.get(rc, 'error')} (status {rc}): {lib.st_last_error().decode(errors='replace')}")
    return n.value, (tiles[0], tiles[1]), np.array(taps, np.float32).reshape(DOF_MAX_SAMPLES, 3)[:n.value].copy()


class FogFalloff(enum.IntEnum):
    """include/strolle_hip.h StFogFalloff: how the fog factor grows with the distance (Bevy's FogFalloff variants)"""
    LINEAR = 0
    EXPONENTIAL = 1
    EXPONENTIAL_SQUARED = 2
    ATMOSPHERIC = 3


class StFogDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("falloff", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32), ("color", C.c_float * 4),
                ("start", C.c_float), ("end", C.c_float), ("density", C.c_float), ("height_falloff", C.c_float), ("height_reference", C.c_float),
                ("sky_distance", C.c_float), ("extinction", C.c_float * 3), ("inscattering", C.c_float * 3), ("light_color", C.c_float * 3),
                ("light_exponent", C.c_float), ("light_direction", C.c_float * 3), ("_pad2", C.c_float)]


FOG_SKY, FOG_FOLLOW_SUN = 1, 2


def fog_desc(falloff=FogFalloff.EXPONENTIAL, color=(1.0, 1.0, 1.0, 1.0), start: float = 0.0, end: float = 100.0, density: float = 0.0,
             height_falloff: float = 0.0, height_reference: float = 0.0, sky_distance=None, extinction=(0.0, 0.0, 0.0), inscattering=(0.0, 0.0, 0.0),
             light_color=(0.0, 0.0, 0.0), light_exponent: float = 8.0, light_direction=(0.0, 1.0, 0.0), follow_sun: bool = False) -> StFogDesc:
    """A StFogDesc (include/strolle_hip.h "fog"). color: linear rgb and the alpha that bounds how much the fog may cover; start / end with
    LINEAR, density with the two exponentials, extinction / inscattering with ATMOSPHERIC; height_falloff 0 = no height dependence;
    sky_distance: None (sky pixels keep their colour) or the distance the sky is fogged at; light_color all 0 = no glow; follow_sun: the
    glow points at the engine's sun instead of light_direction."""
    rgba = tuple(float(v) for v in color) + ((1.0,) if len(color) == 3 else ())
    flags = (FOG_SKY if sky_distance is not None else 0) | (FOG_FOLLOW_SUN if follow_sun else 0)
    f3 = C.c_float * 3
    return StFogDesc(C.sizeof(StFogDesc), int(falloff), flags, 0, (C.c_float * 4)(*rgba), float(start), float(end), float(density), float(height_falloff),
                     float(height_reference), float(sky_distance) if sky_distance is not None else 0.0, f3(*[float(v) for v in extinction]),
                     f3(*[float(v) for v in inscattering]), f3(*[float(v) for v in light_color]), float(light_exponent),
                     f3(*[float(v) for v in light_direction]), 0.0)


class StLensDesc(C.Structure):
    """include/strolle_hip.h "lens effects": 48 B"""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("k1", C.c_float), ("k2", C.c_float), ("scale", C.c_float), ("fringe", C.c_float),
                ("fringe_taps", C.c_uint32), ("vignette_intensity", C.c_float), ("vignette_falloff", C.c_float), ("grain_intensity", C.c_float),
                ("grain_size", C.c_uint32), ("grain_seed", C.c_uint32)]


class StLensPlan(C.Structure):
    """include/strolle_hip.h "lens effects": 284 B"""
    _fields_ = [("steps", C.c_uint32), ("taps", C.c_uint32), ("cx", C.c_float), ("cy", C.c_float), ("inv_hd2", C.c_float), ("fit", C.c_float), ("scale_eff", C.c_float),
                ("tap_scale", C.c_float * 16), ("tap_weight", (C.c_float * 3) * 16)]


LENS_FIT, LENS_VIGNETTE_ROUND, LENS_GRAIN_ANIMATE = 1, 2, 4
LENS_STEP_DISTORTION, LENS_STEP_FRINGE, LENS_STEP_VIGNETTE, LENS_STEP_GRAIN = 1, 2, 4, 8
LENS_MAX_TAPS = 16


def lens_desc(k1: float = 0.0, k2: float = 0.0, scale: float = 1.0, fit: bool = False, fringe: float = 0.0, fringe_taps: int = 3, vignette_intensity: float = 0.0,
              vignette_falloff: float = 1.0, vignette_round: bool = False, grain_intensity: float = 0.0, grain_size: int = 1, grain_seed: int = 0,
              grain_animate: bool = False) -> StLensDesc:
    """A StLensDesc (include/strolle_hip.h "lens effects"); the defaults are neutral. k1, k2: radial distortion (k1 < 0 barrel, > 0
    pincushion), 3 |k1| + 5 |k2| <= 0.95; scale: source zoom, with fit multiplied by the largest factor that keeps every tap inside the
    frame; fringe: the radial spread between red and blue over fringe_taps taps; the vignette follows the frame's ellipse unless
    vignette_round; grain: multiplicative noise of grain_size pixels per cell, a new pattern every frame with grain_animate."""
    flags = (LENS_FIT if fit else 0) | (LENS_VIGNETTE_ROUND if vignette_round else 0) | (LENS_GRAIN_ANIMATE if grain_animate else 0)
    return StLensDesc(C.sizeof(StLensDesc), flags, float(k1), float(k2), float(scale), float(fringe), int(fringe_taps), float(vignette_intensity), float(vignette_falloff),
                      float(grain_intensity), int(grain_size), int(grain_seed) & 0xffffffff)


def lens_plan(desc: StLensDesc, width: int, height: int) -> StLensPlan:
    """st_lens_plan: the host constants of a descriptor for a width x height frame (steps, taps, cx, cy, inv_hd2, fit, scale_eff, the tap table)."""
    lib = load_library()
    lib.st_lens_plan.restype = C.c_int
    lib.st_lens_plan.argtypes = [C.POINTER(StLensDesc), C.c_uint32, C.c_uint32, C.POINTER(StLensPlan)]
    plan = StLensPlan()
    rc = lib.st_lens_plan(C.byref(desc), int(width), int(height), C.byref(plan))
    if rc != 0:
        lib.st_last_error.restype = C.c_char_p
        raise StrolleError(f"{_STATUS.get(rc, 'error')} (status {rc}): {lib.st_last_error().decode(errors='replace')}")
    return plan


class StColorGradingDesc(C.Structure):
    """include/strolle_hip.h "colour grading": 96 B"""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("temperature", C.c_float), ("tint", C.c_float), ("contrast", C.c_float),
                ("saturation", C.c_float), ("slope", C.c_float * 3), ("offset", C.c_float * 3), ("power", C.c_float * 3), ("cdl_saturation", C.c_float),
                ("lut", C.c_uint64), ("lut_domain", C.c_uint32), ("lut_ev_min", C.c_float), ("lut_ev_max", C.c_float), ("lut_strength", C.c_float),
                ("_pad", C.c_uint32 * 2)]


class StColorGradingPlan(C.Structure):
    _fields_ = [("steps", C.c_uint32), ("white_balance", C.c_float * 9), ("lut_inv_range", C.c_float), ("_pad", C.c_uint32)]


class LutDomain(enum.IntEnum):
    """include/strolle_hip.h StLutDomain: what a table's axes span"""
    UNIT = 0
    LOG2 = 1


GRADE_DITHER = 1
GRADE_STEP_WHITE_BALANCE, GRADE_STEP_CONTRAST, GRADE_STEP_SATURATION, GRADE_STEP_CDL, GRADE_STEP_LUT, GRADE_STEP_DITHER = 1, 2, 4, 8, 16, 32


def color_grading_desc(temperature: float = 0.0, tint: float = 0.0, contrast: float = 1.0, saturation: float = 1.0, slope=(1.0, 1.0, 1.0),
                       offset=(0.0, 0.0, 0.0), power=(1.0, 1.0, 1.0), cdl_saturation: float = 1.0, lut: int = 0, lut_domain=LutDomain.UNIT,
                       lut_ev_min: float = -12.0, lut_ev_max: float = 4.0, lut_strength: float = 1.0, dither: bool = False) -> StColorGradingDesc:
    """A StColorGradingDesc (include/strolle_hip.h "colour grading"); the defaults are neutral. temperature, tint: [-1, 1]; contrast and
    saturation grade the scene-referred colour; slope, offset, power, cdl_saturation: an ASC CDL on the display-referred one; lut: a handle
    of Engine.insert_lut (0 = none) read over [0, 1] (UNIT) or over log2 in [lut_ev_min, lut_ev_max] (LOG2); dither: Bevy's DebandDither."""
    f3 = C.c_float * 3
    return StColorGradingDesc(C.sizeof(StColorGradingDesc), GRADE_DITHER if dither else 0, float(temperature), float(tint), float(contrast), float(saturation),
                              f3(*[float(v) for v in slope]), f3(*[float(v) for v in offset]), f3(*[float(v) for v in power]), float(cdl_saturation), int(lut),
                              int(lut_domain), float(lut_ev_min), float(lut_ev_max), float(lut_strength), (C.c_uint32 * 2)(0, 0))


def color_grading_plan(desc: StColorGradingDesc):
    """st_color_grading_plan: (the ST_GRADE_STEP_* bits a frame runs, the white-balance matrix as (3, 3) float32, the LOG2 domain's 1 / range)."""
    import numpy as np
    lib = load_library()
    lib.st_color_grading_plan.restype = C.c_int
    lib.st_color_grading_plan.argtypes = [C.POINTER(StColorGradingDesc), C.POINTER(StColorGradingPlan)]
    plan = StColorGradingPlan()
    rc = lib.st_color_grading_plan(C.byref(desc), C.byref(plan))
    if rc != 0:
        lib.st_last_error.restype = C.c_char_p
        raise StrolleError(f"{_STATUS.get(rc, 'error')} (status {rc}): {lib.st_last_error().decode(errors='replace')}")
    return int(plan.steps), np.array(plan.white_balance, np.float32).reshape(3, 3).copy(), np.float32(plan.lut_inv_range)


class StLightShaftsDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("steps", C.c_uint32), ("divisor", C.c_uint32),
                ("density", C.c_float), ("anisotropy", C.c_float), ("max_distance", C.c_float), ("intensity", C.c_float),
                ("scatter", C.c_float * 3), ("_pad", C.c_float), ("sun_color", C.c_float * 3), ("_pad2", C.c_float),
                ("sun_direction", C.c_float * 3), ("light_count", C.c_uint32), ("lights", C.c_uint64 * 8)]


SHAFTS_FOLLOW_SUN, SHAFTS_LIGHT_EXTINCTION, SHAFTS_MAX_LIGHTS = 1, 2, 8


def light_shafts_desc(steps: int = 16, divisor: int = 2, density: float = 0.05, anisotropy: float = 0.0, max_distance: float = 100.0, intensity: float = 1.0,
                      scatter=(1.0, 1.0, 1.0), sun_color=(0.0, 0.0, 0.0), sun_direction=(0.0, 1.0, 0.0), lights=(), follow_sun: bool = False,
                      light_extinction: bool = False) -> StLightShaftsDesc:
    """A StLightShaftsDesc (include/strolle_hip.h "light shafts"). steps: samples per ray (1..64); divisor: pixels per cell side (1 or 2);
    density: extinction per metre; anisotropy: Henyey-Greenstein g; scatter: single-scattering albedo; sun_color all 0 = no sun;
    follow_sun: the sun's direction is the engine's instead of sun_direction; lights: up to 8 light handles; light_extinction: the medium
    also attenuates the light on its way from a light to the sample."""
    handles = [int(h) for h in lights]
    flags = (SHAFTS_FOLLOW_SUN if follow_sun else 0) | (SHAFTS_LIGHT_EXTINCTION if light_extinction else 0)
    f3 = C.c_float * 3
    return StLightShaftsDesc(C.sizeof(StLightShaftsDesc), flags, int(steps), int(divisor), float(density), float(anisotropy), float(max_distance), float(intensity),
                             f3(*[float(v) for v in scatter]), 0.0, f3(*[float(v) for v in sun_color]), 0.0, f3(*[float(v) for v in sun_direction]),
                             len(handles), (C.c_uint64 * 8)(*(handles[:8] + [0] * (8 - min(len(handles), 8)))))


def light_shafts_plan(desc: StLightShaftsDesc, width: int, height: int):
    """st_light_shafts_plan: ((cells_w, cells_h), the 4 x 4 jitter table, row cy & 3, column cx & 3)."""
    import numpy as np
    lib = load_library()
    lib.st_light_shafts_plan.restype = C.c_int
    lib.st_light_shafts_plan.argtypes = [C.POINTER(StLightShaftsDesc), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    cells, jitter = (C.c_uint32 * 2)(), (C.c_float * 16)()
    rc = lib.st_light_shafts_plan(C.byref(desc), width, height, cells, jitter)
    if rc != 0:
        lib.st_last_error.restype = C.c_char_p
        raise StrolleError(f"{_STATUS.get(rc, 'error')} (status {rc}): {lib.st_last_error().decode(errors='replace')}")
    return (cells[0], cells[1]), np.array(jitter, np.float32).reshape(4, 4).copy()


class StBloomDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("levels", C.c_uint32), ("intensity", C.c_float),
                ("low_frequency_boost", C.c_float), ("low_frequency_boost_curvature", C.c_float), ("high_pass_frequency", C.c_float),
                ("threshold", C.c_float), ("threshold_softness", C.c_float), ("clamp", C.c_float)]


BLOOM_ADDITIVE = 1
BLOOM_FIREFLY_SUPPRESS = 2
BLOOM_MAX_LEVELS = 8


def bloom_desc(intensity: float = 0.15, additive: bool = False, firefly_suppress: bool = False, levels: int = 0, low_frequency_boost: float = 0.7,
               low_frequency_boost_curvature: float = 0.95, high_pass_frequency: float = 1.0, threshold: float = 0.0, threshold_softness: float = 0.0,
               clamp: float = 0.0) -> StBloomDesc:
    """A StBloomDesc; the defaults are Bevy's "natural" bloom (energy conserving, no threshold). levels 0 = 6, clamp 0 = 65504
    (include/strolle_hip.h "bloom")."""
    return StBloomDesc(C.sizeof(StBloomDesc), (BLOOM_ADDITIVE if additive else 0) | (BLOOM_FIREFLY_SUPPRESS if firefly_suppress else 0), int(levels),
                       float(intensity), float(low_frequency_boost), float(low_frequency_boost_curvature), float(high_pass_frequency),
                       float(threshold), float(threshold_softness), float(clamp))


class StRay(C.Structure):
    """include/strolle_hip.h StRay (32 B): hits count for 0 < t < t_max; the direction is used as given (t in units of |direction|)."""
    _fields_ = [("origin", C.c_float * 3), ("t_max", C.c_float), ("direction", C.c_float * 3), ("_pad", C.c_uint32)]


class StRayHit(C.Structure):
    """include/strolle_hip.h StRayHit (64 B): t = FLT_MAX and everything else 0 on a miss."""
    _fields_ = [("point", C.c_float * 3), ("t", C.c_float), ("normal", C.c_float * 3), ("triangle", C.c_uint32),
                ("uv", C.c_float * 2), ("barycentric", C.c_float * 2), ("instance", C.c_uint64), ("hit", C.c_uint32), ("_pad", C.c_uint32)]


# numpy records of the same layout (arrays of them are what the scene queries read and write)
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("t_max", "<f4"), ("direction", "<f4", (3,)), ("_pad", "<u4")])
HIT_DTYPE = np.dtype([("point", "<f4", (3,)), ("t", "<f4"), ("normal", "<f4", (3,)), ("triangle", "<u4"), ("uv", "<f4", (2,)),
                      ("barycentric", "<f4", (2,)), ("instance", "<u8"), ("hit", "<u4"), ("_pad", "<u4")])
RAY_COHERENT = 1   # ST_RAY_COHERENT
RAY_MAPPED_NORMAL = 2   # ST_RAY_MAPPED_NORMAL


class Aov(enum.IntEnum):
    """StAovKind: the per-pixel AOV planes of st_camera_render_aovs (include/strolle_hip.h "per-pixel AOVs")."""
    DEPTH = 0      # f32: distance from the camera ray's origin to the hit; FLT_MAX on sky
    NORMAL = 1     # f32x4: shading normal (xyz), w = 0; 0 on sky
    ALBEDO = 2     # f32x4: linear base colour at the hit, texture applied, alpha in w; 0 on sky
    MOTION = 3     # f32x2: the renderer's velocity (current minus previous screen position); 0 on sky
    INSTANCE = 4   # u64: st_instance_insert handle; 0 on sky
    TRIANGLE = 5   # u32: index into the mesh's st_mesh_insert array; 0xffffffff on sky


AOV_COUNT = 6


class StAovTargets(C.Structure):
    """include/strolle_hip.h StAovTargets (56 B): one device pointer per Aov, width x height elements, row-major; NULL = not wanted."""
    _fields_ = [("struct_size", C.c_uint32), ("_pad", C.c_uint32), ("planes", C.c_void_p * AOV_COUNT)]


# element of one pixel of each plane: (numpy scalar type, components per pixel)
AOV_ELEMENT = {Aov.DEPTH: (np.float32, 1), Aov.NORMAL: (np.float32, 4), Aov.ALBEDO: (np.float32, 4), Aov.MOTION: (np.float32, 2),
               Aov.INSTANCE: (np.uint64, 1), Aov.TRIANGLE: (np.uint32, 1)}


def aov_planes(size, kinds=tuple(Aov), device="cuda", fill=None) -> dict:
    """Torch planes for Engine.render_aovs of a camera of `size` = (width, height) (or a Camera): {Aov: tensor of shape (height,
    width[, components])} on `device`, typed as the header says. fill=None leaves them uninitialised; otherwise every element is `fill`."""
    import torch
    w, h = (size.size if isinstance(size, Camera) else size)
    dtypes = {np.float32: torch.float32, np.uint64: torch.uint64, np.uint32: torch.uint32}
    out = {}
    for k in kinds:
        k = Aov(k)
        scalar, comps = AOV_ELEMENT[k]
        shape = (int(h), int(w)) if comps == 1 else (int(h), int(w), comps)
        t = torch.empty(shape, dtype=dtypes[scalar], device=device)
        if fill is not None:
            t.fill_(fill)
        out[k] = t
    return out


class StrolleError(RuntimeError):
    pass


class OutputFormat(enum.IntEnum):
    """StOutputFormat"""
    RGBA32F = 0
    RGBA16F = 1
    RGBA8_UNORM_SRGB = 2
    BGRA8_UNORM_SRGB = 3


class Buffer(enum.IntEnum):
    """Per-camera buffers (strolle/src/camera_controller/buffers.rs:7-51); values == StBufferId."""
    PRIM_GBUFFER_D0_A = 0; PRIM_GBUFFER_D0_B = 1; PRIM_GBUFFER_D1_A = 2; PRIM_GBUFFER_D1_B = 3
    PRIM_SURFACE_MAP_A = 4; PRIM_SURFACE_MAP_B = 5; REPROJECTION_MAP = 6; VELOCITY_MAP = 7
    DI_RESERVOIRS_0 = 8; DI_RESERVOIRS_1 = 9; DI_RESERVOIRS_2 = 10
    DI_DIFF_SAMPLES = 11; DI_DIFF_PREV_COLORS = 12; DI_DIFF_CURR_COLORS = 13
    DI_DIFF_MOMENTS_A = 14; DI_DIFF_MOMENTS_B = 15; DI_DIFF_STASH = 16; DI_SPEC_SAMPLES = 17
    GI_D0 = 18; GI_D1 = 19; GI_D2 = 20
    GI_RESERVOIRS_0 = 21; GI_RESERVOIRS_1 = 22; GI_RESERVOIRS_2 = 23; GI_RESERVOIRS_3 = 24
    GI_DIFF_SAMPLES = 25; GI_DIFF_PREV_COLORS = 26; GI_DIFF_CURR_COLORS = 27
    GI_DIFF_MOMENTS_A = 28; GI_DIFF_MOMENTS_B = 29; GI_DIFF_STASH = 30; GI_SPEC_SAMPLES = 31
    REF_HITS = 32; REF_RAYS = 33; REF_COLORS = 34; DBG_USED_MEMORY = 35


class PassBit(enum.IntFlag):
    """StPassBit: one bit per reference pass (camera_controller.rs:87-174 order)."""
    PRIM_VISIBILITY = 1 << 0; FRAME_REPROJECTION = 1 << 1
    DI_SAMPLING = 1 << 2; DI_TEMPORAL = 1 << 3; DI_SPATIAL_PICK = 1 << 4; DI_SPATIAL_TRACE = 1 << 5; DI_SPATIAL_SAMPLE = 1 << 6; DI_RESOLVING = 1 << 7
    GI_REPROJECTION = 1 << 8; GI_SAMPLING_A = 1 << 9; GI_SAMPLING_B = 1 << 10; GI_TEMPORAL = 1 << 11
    GI_SPATIAL_PICK = 1 << 12; GI_SPATIAL_TRACE = 1 << 13; GI_SPATIAL_SAMPLE = 1 << 14
    GI_PREVIEW_0 = 1 << 15; GI_PREVIEW_1 = 1 << 16; GI_RESOLVING = 1 << 17
    DENOISE_REPROJECT_DI = 1 << 18; DENOISE_REPROJECT_GI = 1 << 19; DENOISE_VARIANCE = 1 << 20
    DENOISE_WAVELET_0 = 1 << 21; DENOISE_WAVELET_1 = 1 << 22; DENOISE_WAVELET_2 = 1 << 23; DENOISE_WAVELET_3 = 1 << 24; DENOISE_WAVELET_4 = 1 << 25
    COMPOSITION = 1 << 26; BVH_HEATMAP = 1 << 27; REF_TRACING = 1 << 28; REF_SHADING = 1 << 29; POST = 1 << 30


# ----------------------------------------------------------------------------- value types mirroring the reference
class CameraMode(enum.IntEnum):
    """strolle/src/camera.rs:83-105"""
    IMAGE = 0; DI_DIFFUSE = 1; DI_SPECULAR = 2; GI_DIFFUSE = 3; GI_SPECULAR = 4; BVH_HEATMAP = 5; REFERENCE = 6


@dataclasses.dataclass
class Camera:
    """strolle/src/camera.rs:8-14. `transform`/`projection` are 4x4 numpy arrays in maths layout
    (m[row, col]); they are handed over column-major like glam's Mat4."""
    mode: CameraMode = CameraMode.IMAGE
    denoise: bool = True
    depth: int = 0
    size: tuple = (512, 512)
    position: tuple = (0, 0)
    transform: np.ndarray = dataclasses.field(default_factory=lambda: np.eye(4, dtype=np.float32))
    projection: np.ndarray = dataclasses.field(default_factory=lambda: np.eye(4, dtype=np.float32))

    def to_c(self) -> StCamera:
        c = StCamera()
        c.mode = int(self.mode); c.denoise = 1 if self.denoise else 0; c.depth = int(self.depth)
        c.width, c.height = int(self.size[0]), int(self.size[1])
        c.pos_x, c.pos_y = int(self.position[0]), int(self.position[1])
        c.transform[:] = np.asarray(self.transform, dtype=np.float32).T.reshape(-1).tolist()
        c.projection[:] = np.asarray(self.projection, dtype=np.float32).T.reshape(-1).tolist()
        return c


@dataclasses.dataclass
class Material:
    """strolle/src/material.rs:8-70 (defaults :53-70)."""
    base_color: Sequence[float] = (1.0, 1.0, 1.0, 1.0)
    base_color_texture: Optional[int] = None
    emissive: Sequence[float] = (0.0, 0.0, 0.0, 0.0)
    emissive_texture: Optional[int] = None
    perceptual_roughness: float = 0.5
    metallic: float = 0.0
    metallic_roughness_texture: Optional[int] = None
    reflectance: float = 0.5
    ior: float = 1.0
    normal_map_texture: Optional[int] = None
    alpha_mode: int = 0  # 0 Opaque, 1 Blend

    def to_c(self) -> StMaterial:
        m = StMaterial()
        m.base_color[:] = [float(x) for x in self.base_color]
        m.emissive[:] = [float(x) for x in self.emissive]
        m.perceptual_roughness = self.perceptual_roughness; m.metallic = self.metallic
        m.reflectance = self.reflectance; m.ior = self.ior
        m.base_color_texture = self.base_color_texture or 0
        m.emissive_texture = self.emissive_texture or 0
        m.metallic_roughness_texture = self.metallic_roughness_texture or 0
        m.normal_map_texture = self.normal_map_texture or 0
        m.alpha_mode = self.alpha_mode
        return m


@dataclasses.dataclass
class Light:
    """strolle/src/light.rs:6-22"""
    kind: int
    position: Sequence[float]
    radius: float
    color: Sequence[float]
    range: float
    direction: Sequence[float] = (0.0, 0.0, 0.0)
    angle: float = 0.0

    @staticmethod
    def point(position, radius, color, range) -> "Light":
        return Light(0, position, radius, color, range)

    @staticmethod
    def spot(position, radius, color, range, direction, angle) -> "Light":
        return Light(1, position, radius, color, range, direction, angle)

    def to_c(self) -> StLight:
        l = StLight()
        l.kind = self.kind; l.position[:] = [float(x) for x in self.position]; l.radius = self.radius
        l.color[:] = [float(x) for x in self.color]; l.range = self.range
        l.direction[:] = [float(x) for x in self.direction]; l.angle = self.angle
        return l


@dataclasses.dataclass
class Sun:
    """strolle/src/sun.rs:1-14"""
    azimuth: float = 0.0
    altitude: float = 0.35


class Mesh:
    """strolle/src/mesh.rs + mesh_triangle.rs: object-space triangles.
    positions/normals: [n,3,3] float32, uvs: [n,3,2], tangents: [n,3,4] (optional)."""

    def __init__(self, positions, normals, uvs=None, tangents=None):
        self.positions = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3, 3)
        n = len(self.positions)
        self.normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(n, 3, 3)
        self.uvs = np.zeros((n, 3, 2), np.float32) if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(n, 3, 2)
        self.tangents = np.zeros((n, 3, 4), np.float32) if tangents is None else np.ascontiguousarray(tangents, dtype=np.float32).reshape(n, 3, 4)

    def pack(self) -> np.ndarray:
        n = len(self.positions)
        out = np.concatenate([self.positions.reshape(n, 9), self.normals.reshape(n, 9), self.uvs.reshape(n, 6), self.tangents.reshape(n, 12)], axis=1)
        return np.ascontiguousarray(out, dtype=np.float32)


@dataclasses.dataclass
class Instance:
    """strolle/src/instance.rs:16-31. transform: glam Affine3A as a 3x4 numpy array [R | t]."""
    mesh_handle: int
    material_handle: int
    transform: np.ndarray

    def xform12(self):
        t = np.asarray(self.transform, dtype=np.float32).reshape(3, 4)
        return np.concatenate([t[:, 0], t[:, 1], t[:, 2], t[:, 3]]).astype(np.float32)


# ----------------------------------------------------------------------------- camera matrices (what Bevy hands to the engine)
def perspective_infinite_reverse_rh(fov_y: float, aspect: float, z_near: float) -> np.ndarray:
    """glam Mat4::perspective_infinite_reverse_rh — Bevy's PerspectiveProjection (default fov pi/4, near 0.1)."""
    f = np.float32(1.0 / math.tan(0.5 * fov_y))
    m = np.zeros((4, 4), np.float32)
    m[0, 0] = np.float32(f / np.float32(aspect)); m[1, 1] = f; m[3, 2] = -1.0; m[2, 3] = np.float32(z_near)
    return m


def look_at_transform(eye, target, up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """World transform of a camera at `eye` looking at `target` (Bevy Transform::looking_at), 4x4."""
    eye = np.asarray(eye, np.float64); target = np.asarray(target, np.float64); up = np.asarray(up, np.float64)
    back = eye - target; back /= np.linalg.norm(back)
    right = np.cross(up, back); right /= np.linalg.norm(right)
    upv = np.cross(back, right)
    m = np.eye(4)
    m[:3, 0] = right; m[:3, 1] = upv; m[:3, 2] = back; m[:3, 3] = eye
    return m.astype(np.float32)


# ----------------------------------------------------------------------------- binding
class _Binding:
    """Function table over a C library exporting `<prefix>engine_create` etc."""

    def __init__(self, lib: C.CDLL, prefix: str, has_device: bool):
        self.lib, self.prefix, self.has_device = lib, prefix, has_device
        u64, vp, i32, u32, sz = C.c_uint64, C.c_void_p, C.c_int, C.c_uint32, C.c_size_t
        P = C.POINTER

        def fn(name, args):
            f = getattr(lib, prefix + name)
            f.restype = i32
            f.argtypes = args
            return f

        self.engine_create = fn("engine_create", [i32, P(vp)] if has_device else [P(vp)])
        self.engine_destroy = getattr(lib, prefix + "engine_destroy"); self.engine_destroy.restype = None; self.engine_destroy.argtypes = [vp]
        self.mesh_insert = fn("mesh_insert", [vp, u64, vp, sz]); self.mesh_remove = fn("mesh_remove", [vp, u64])
        self.material_insert = fn("material_insert", [vp, u64, P(StMaterial)]); self.material_has = fn("material_has", [vp, u64])
        self.material_remove = fn("material_remove", [vp, u64])
        self.instance_insert = fn("instance_insert", [vp, u64, u64, u64, P(C.c_float)]); self.instance_remove = fn("instance_remove", [vp, u64])
        self.light_insert = fn("light_insert", [vp, u64, P(StLight)]); self.light_remove = fn("light_remove", [vp, u64])
        self.sun_update = fn("sun_update", [vp, C.c_float, C.c_float])
        self.camera_create = fn("camera_create", [vp, P(StCamera), P(u64)]); self.camera_update = fn("camera_update", [vp, u64, P(StCamera)])
        self.camera_delete = fn("camera_delete", [vp, u64])
        self.tick = fn("tick", [vp, vp] if has_device else [vp])
        self.render_camera = fn("render_camera", [vp, u64, vp, vp] if has_device else [vp, u64, vp])
        self.set_seed = fn("set_seed", [vp, u64]); self.set_blue_noise = fn("set_blue_noise", [vp, vp, sz])
        self.debug_read_lut = fn("debug_read_lut", [vp, i32, vp, sz, P(sz)])
        self.camera_read_buffer = fn("camera_read_buffer", [vp, u64, i32, vp, sz, P(sz)])
        self.camera_ray_count = fn("camera_ray_count", [vp, u64, P(u64), i32])
        self.debug_read_scene = fn("debug_read_scene", [vp, i32, vp, sz, P(sz)])
        self.debug_world = fn("debug_world", [vp, P(u32), P(u32)])
        self.debug_image_rect = fn("debug_image_rect", [vp, u64, P(u32)])
        self.set_bvh_refresh = fn("set_bvh_refresh", [vp, i32]); self.debug_bvh_refits = fn("debug_bvh_refits", [vp, P(u64), P(u64)])
        if has_device:
            self.debug_bvh_depth = fn("debug_bvh_depth", [vp, P(u32), P(u32)])
            if hasattr(lib, prefix + "debug_walk_overflow"):   # (round 6; a round-5 library loaded for a same-box A/B has none)
                self.debug_walk_overflow = fn("debug_walk_overflow", [vp, P(u64), P(u32), P(u32)])
            self.debug_bvh_device_refits = fn("debug_bvh_device_refits", [vp, P(u64)])
            self.debug_device_bakes = fn("debug_device_bakes", [vp, P(u64), P(u64)])
            if hasattr(lib, prefix + "debug_auto_tree"):   # (round 6, late)
                self.debug_auto_tree = fn("debug_auto_tree", [vp, P(C.c_float), P(u32)])
            self.debug_device_builds = fn("debug_device_builds", [vp, P(u64)])
            self.debug_device_tree_refits = fn("debug_device_tree_refits", [vp, P(u64)])
            self.engine_get_tuning = fn("engine_get_tuning", [vp, P(StTuning)]); self.engine_set_tuning = fn("engine_set_tuning", [vp, P(StTuning)])
            self.debug_copy_bandwidth = fn("debug_copy_bandwidth", [vp, sz, i32, P(C.c_double)])
            self.debug_variance_flags = fn("debug_variance_flags", [vp, u64, vp, sz, P(sz)])
            self.camera_set_window = fn("camera_set_window", [vp, u64, u32, u32, u32, u32])
            self.dist_init = fn("dist_init", [vp, i32, i32, P(StDistUniqueId)]); self.dist_init_local = fn("dist_init_local", [vp, i32, i32, u64])
            self.dist_shutdown = fn("dist_shutdown", [vp]); self.dist_rank = fn("dist_rank", [vp, P(i32), P(i32)])
            self.dist_set_partition = fn("dist_set_partition", [vp, u64, u32, u32, P(StDistRect), P(StDistRect)])
            self.dist_set_grid = fn("dist_set_grid", [vp, u64, P(StDistGrid), u32, P(StDistRect), P(StDistRect)])
            self.dist_gather = fn("dist_gather", [vp, u64, vp, vp, vp]); self.dist_wait = fn("dist_wait", [vp, u64, vp, vp, i32])
            self.dist_gather_ms = fn("dist_gather_ms", [vp, u64, P(C.c_float)])
        self.image_insert_rgba8 = fn("image_insert_rgba8", [vp, u64, u32, u32, vp, i32]); self.image_remove = fn("image_remove", [vp, u64])
        if hasattr(lib, prefix + "environment_set"):   # environment lighting (absent from an older library)
            self.environment_set = fn("environment_set", [vp, vp, u32, u32, u32, P(StEnvironmentDesc)])
            self.environment_set_device = fn("environment_set_device", [vp, vp, u32, u32, u32, sz, P(StEnvironmentDesc)])
            self.environment_update = fn("environment_update", [vp, P(StEnvironmentDesc)])
            self.environment_clear = fn("environment_clear", [vp])
            self.debug_environment_eval = fn("debug_environment_eval", [vp, vp, u32, vp, vp])
            self.debug_environment_sample = fn("debug_environment_sample", [vp, vp, u32, vp, vp])
            self.debug_environment_pdf = fn("debug_environment_pdf", [vp, vp, u32, vp, vp])
            self.debug_environment_sanitized = fn("debug_environment_sanitized", [vp, P(u64)])
            self.debug_environment_table = fn("debug_environment_table", [vp, vp, sz, P(u32), P(u32)])
        if hasattr(lib, prefix + "camera_set_display"):   # display transforms (likewise absent from an older library)
            self.camera_set_display = fn("camera_set_display", [vp, u64, P(StDisplayDesc)])
            self.camera_get_display = fn("camera_get_display", [vp, u64, P(StDisplayDesc), P(i32)])
            self.camera_exposure = fn("camera_exposure", [vp, u64, P(C.c_float), P(C.c_float), P(C.c_float)])
            self.debug_camera_histogram = fn("debug_camera_histogram", [vp, u64, P(u32)])
        if hasattr(lib, prefix + "camera_set_post"):   # output post-processing (likewise)
            self.camera_set_post = fn("camera_set_post", [vp, u64, P(StPostDesc)])
            self.camera_get_post = fn("camera_get_post", [vp, u64, P(StPostDesc), P(i32)])
            self.camera_output_size = fn("camera_output_size", [vp, u64, P(u32), P(u32)])
            self.post_process = fn("post_process", [vp, P(StPostDesc), vp, u32, u32, vp, i32, vp])
        if hasattr(lib, prefix + "camera_set_upscale"):   # the upscale stage (likewise)
            self.camera_set_upscale = fn("camera_set_upscale", [vp, u64, P(StUpscaleDesc)])
            self.camera_get_upscale = fn("camera_get_upscale", [vp, u64, P(StUpscaleDesc), P(i32)])
            self.upscale_process = fn("upscale_process", [vp, P(StUpscaleDesc), vp, u32, u32, vp, i32, vp])
            self.debug_set_upscale_fused = fn("debug_set_upscale_fused", [vp, i32])
        if hasattr(lib, prefix + "camera_set_bloom"):   # bloom (likewise)
            self.camera_set_bloom = fn("camera_set_bloom", [vp, u64, P(StBloomDesc)])
            self.camera_get_bloom = fn("camera_get_bloom", [vp, u64, P(StBloomDesc), P(i32)])
            self.bloom_plan = fn("bloom_plan", [P(StBloomDesc), u32, u32, P(u32), P(u32), P(C.c_float)])
            self.debug_set_bloom_tail = fn("debug_set_bloom_tail", [vp, i32, P(u32)])
            self.bloom_process = fn("bloom_process", [vp, P(StBloomDesc), P(StDisplayDesc), vp, u32, u32, vp, i32, vp])
        if hasattr(lib, prefix + "camera_set_motion_blur"):   # motion blur (likewise)
            self.camera_set_motion_blur = fn("camera_set_motion_blur", [vp, u64, P(StMotionBlurDesc)])
            self.camera_get_motion_blur = fn("camera_get_motion_blur", [vp, u64, P(StMotionBlurDesc), P(i32)])
            self.motion_blur_process = fn("motion_blur_process", [vp, P(StMotionBlurDesc), P(StDisplayDesc), vp, vp, vp, u32, u32, vp, i32, vp])
        if hasattr(lib, prefix + "camera_set_dof"):   # depth of field (likewise)
            self.camera_set_dof = fn("camera_set_dof", [vp, u64, P(StDofDesc)])
            self.camera_get_dof = fn("camera_get_dof", [vp, u64, P(StDofDesc), P(i32)])
            self.dof_plan = fn("dof_plan", [P(StDofDesc), u32, u32, P(u32), P(u32), P(C.c_float)])
            self.dof_process = fn("dof_process", [vp, P(StDofDesc), P(StDisplayDesc), P(C.c_float), vp, vp, u32, u32, vp, i32, vp])
        if hasattr(lib, prefix + "camera_set_fog"):   # fog (likewise)
            self.camera_set_fog = fn("camera_set_fog", [vp, u64, P(StFogDesc)])
            self.camera_get_fog = fn("camera_get_fog", [vp, u64, P(StFogDesc), P(i32)])
            self.fog_process = fn("fog_process", [vp, P(StFogDesc), P(StDisplayDesc), P(C.c_float), P(C.c_float), vp, vp, u32, u32, vp, i32, vp])
        if hasattr(lib, prefix + "camera_set_lens"):   # lens effects (likewise)
            self.camera_set_lens = fn("camera_set_lens", [vp, u64, P(StLensDesc)])
            self.camera_get_lens = fn("camera_get_lens", [vp, u64, P(StLensDesc), P(i32)])
            self.lens_plan = fn("lens_plan", [P(StLensDesc), u32, u32, P(StLensPlan)])
            self.lens_process = fn("lens_process", [vp, P(StLensDesc), P(StDisplayDesc), vp, u32, u32, vp, i32, vp])
            self.debug_set_lens_gather = fn("debug_set_lens_gather", [vp, i32])
        if hasattr(lib, prefix + "camera_set_color_grading"):   # colour grading (likewise)
            self.camera_set_color_grading = fn("camera_set_color_grading", [vp, u64, P(StColorGradingDesc)])
            self.camera_get_color_grading = fn("camera_get_color_grading", [vp, u64, P(StColorGradingDesc), P(i32)])
            self.color_grading_plan = fn("color_grading_plan", [P(StColorGradingDesc), P(StColorGradingPlan)])
            self.color_grading_process = fn("color_grading_process", [vp, P(StColorGradingDesc), P(StDisplayDesc), vp, u32, vp, u32, u32, vp, i32, vp])
            self.lut_insert = fn("lut_insert", [vp, u64, u32, P(C.c_float)]); self.lut_remove = fn("lut_remove", [vp, u64])
        if hasattr(lib, prefix + "camera_set_light_shafts"):   # light shafts (likewise)
            self.camera_set_light_shafts = fn("camera_set_light_shafts", [vp, u64, P(StLightShaftsDesc)])
            self.camera_get_light_shafts = fn("camera_get_light_shafts", [vp, u64, P(StLightShaftsDesc), P(i32)])
            self.light_shafts_process = fn("light_shafts_process", [vp, P(StLightShaftsDesc), P(StDisplayDesc), P(C.c_float), P(C.c_float), vp, vp, u32, u32, vp, i32, vp])
        if hasattr(lib, prefix + "mesh_set_skin"):
            self.mesh_set_skin = fn("mesh_set_skin", [vp, u64, vp, sz, u32])
        if hasattr(lib, prefix + "mesh_set_morph_targets"):   # morph targets (likewise absent from an older library)
            self.mesh_set_morph_targets = fn("mesh_set_morph_targets", [vp, u64, vp, sz, u32])
            self.instance_set_morph_weights = fn("instance_set_morph_weights", [vp, u64, P(C.c_float), u32])
            self.debug_morphing = fn("debug_morphing", [vp, P(u64), P(u64), P(u64)])
        if hasattr(lib, prefix + "engine_set_deformation_motion"):   # deformation motion (likewise absent from an older library)
            self.engine_set_deformation_motion = fn("engine_set_deformation_motion", [vp, i32])
            self.engine_get_deformation_motion = fn("engine_get_deformation_motion", [vp, P(i32)])
            self.debug_deformation = fn("debug_deformation", [vp, P(u64), P(u64)])
        if hasattr(lib, prefix + "engine_set_normal_mapping"):   # normal mapping (likewise)
            self.engine_set_normal_mapping = fn("engine_set_normal_mapping", [vp, i32])
            self.engine_get_normal_mapping = fn("engine_get_normal_mapping", [vp, P(i32)])
        if has_device:
            self.camera_set_rows = fn("camera_set_rows", [vp, u64, u32, u32])
            self.camera_set_output_format = fn("camera_set_output_format", [vp, u64, i32])
            self.image_insert_device_rgba8 = fn("image_insert_device_rgba8", [vp, u64, u32, u32, vp, sz, i32])
            self.debug_bvh_refresh = fn("debug_bvh_refresh", [vp, P(u64), P(u64)])
            self.scene_load_gltf = fn("scene_load_gltf", [vp, C.c_char_p, P(StGltfOptions), P(StGltfSummary)])
            self.scene_load_gltf_memory = fn("scene_load_gltf_memory", [vp, vp, sz, C.c_char_p, P(StGltfOptions), P(StGltfSummary)])
            self.decode_png = fn("decode_png", [vp, sz, vp, sz, P(u32), P(u32)])
            self.engine_set_arithmetic = fn("engine_set_arithmetic", [vp, i32]); self.engine_get_arithmetic = fn("engine_get_arithmetic", [vp, P(i32)])
            self.camera_write_buffer = fn("camera_write_buffer", [vp, u64, i32, vp, sz])
            self.debug_set_pass_mask = fn("debug_set_pass_mask", [vp, u64]); self.debug_set_launch_filter = fn("debug_set_launch_filter", [vp, u64]); self.debug_last_launches = fn("debug_last_launches", [vp, P(u64), sz, P(sz)])
            self.debug_keep_all_planes = fn("debug_keep_all_planes", [vp, i32])
            self.camera_buffer_stale = fn("camera_buffer_stale", [vp, u64, i32, P(i32)])
            self.camera_present_copy = fn("camera_present_copy", [vp, u64, vp, vp, sz, vp])
            self.camera_present_ready = fn("camera_present_ready", [vp, u64, vp, i32, P(i32)])
            if hasattr(lib, prefix + "scene_trace_rays"):   # scene queries (a library built before them, loaded for a same-box A/B, has none)
                self.scene_trace_rays = fn("scene_trace_rays", [vp, vp, u32, vp, u32, vp])
                self.scene_occluded = fn("scene_occluded", [vp, vp, u32, vp, vp])
                self.camera_pick = fn("camera_pick", [vp, u64, vp, u32, vp, vp])
                self.scene_trace_rays_host = fn("scene_trace_rays_host", [vp, vp, u32, vp])
            if hasattr(lib, prefix + "camera_render_aovs"):   # per-pixel AOVs (likewise absent from an older library)
                self.camera_render_aovs = fn("camera_render_aovs", [vp, u64, P(StAovTargets), vp])
            if hasattr(lib, prefix + "instance_set_pose"):   # skinned meshes (likewise absent from an older library)
                self.instance_set_pose = fn("instance_set_pose", [vp, u64, P(C.c_float), u32])
                self.debug_skinning = fn("debug_skinning", [vp, P(u64), P(u64), P(u64)])
                self.debug_read_posed = fn("debug_read_posed", [vp, u64, P(C.c_float), sz, P(sz)])
            self.profile_enable = fn("profile_enable", [vp, i32])
            self.profile_read = fn("profile_read", [vp, P(StKernelProfile), sz, P(sz), i32])
            self.last_error = getattr(lib, prefix + "last_error"); self.last_error.restype = C.c_char_p; self.last_error.argtypes = []


_STATUS = {1: "invalid argument", 2: "no HIP device (host-only engine or HIP unavailable)", 3: "camera does not exist",
           4: "mesh contains no triangles", 5: "HIP runtime error", 6: "no more space in the atlas", 7: "file could not be read",
           8: "malformed scene file", 9: "unsupported scene file feature",
           10: "the BVH is deeper than the kernels' traversal stack (the scene was uploaded; pushes beyond 24 pending entries are dropped)",
           11: "collective transport error"}
ST_ERR_BVH_TOO_DEEP = 10


class EngineBase:
    """Shared call sequence; `Engine` binds it to libstrolle_hip.so."""

    def __init__(self, binding: _Binding, device: int = 0):
        self._b = binding
        h = C.c_void_p()
        self._check(binding.engine_create(device, C.byref(h)) if binding.has_device else binding.engine_create(C.byref(h)))
        self._h = h
        self._keep = []

    def _check(self, status: int):
        if status != 0:
            detail = ""
            if self._b.has_device:
                msg = self._b.last_error()
                detail = f": {msg.decode(errors='replace')}" if msg else ""
            raise StrolleError(f"{_STATUS.get(status, 'error')} (status {status}){detail}")

    def close(self):
        if getattr(self, "_h", None):
            self._b.engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- scene (lib.rs:161-246)
    def insert_mesh(self, handle: int, mesh: Mesh):
        data = mesh.pack()
        self._check(self._b.mesh_insert(self._h, handle, data.ctypes.data, len(data)))

    def remove_mesh(self, handle: int):
        self._check(self._b.mesh_remove(self._h, handle))

    def set_skin(self, mesh: int, joints, weights, joint_count: int):
        """st_mesh_set_skin: joints (3n, 4) joint indices and weights (3n, 4) per corner of mesh `mesh`'s n triangles (corner v of
        triangle t at row 3 t + v); weights are used as given."""
        joints = np.asarray(joints).reshape(-1, 4); weights = np.asarray(weights, np.float32).reshape(-1, 4)
        corners = np.zeros(len(joints), SKIN_VERTEX_DTYPE)
        corners["joints"] = joints; corners["weights"] = weights
        self._check(self._b.mesh_set_skin(self._h, mesh, corners.ctypes.data if len(corners) else None, len(corners), joint_count))

    def set_morph_targets(self, mesh: int, position_deltas, normal_deltas):
        """st_mesh_set_morph_targets: position and normal deltas, each (K, n, 3, 3), of K targets over mesh `mesh`'s n triangles (corner v of
        triangle t of target k at [k, t, v])."""
        dp = np.asarray(position_deltas, np.float32); dn = np.asarray(normal_deltas, np.float32)
        if dp.ndim != 4 or dp.shape[2:] != (3, 3) or dn.shape != dp.shape:
            raise StrolleError("morph deltas: expected two arrays of shape (K, n, 3, 3)")
        deltas = np.zeros((dp.shape[0], dp.shape[1] * 3), MORPH_DELTA_DTYPE)
        deltas["position"] = dp.reshape(dp.shape[0], -1, 3); deltas["normal"] = dn.reshape(dp.shape[0], -1, 3)
        self._check(self._b.mesh_set_morph_targets(self._h, mesh, deltas.ctypes.data if deltas.size else None, deltas.shape[1], deltas.shape[0]))

    def insert_material(self, handle: int, material: Material):
        m = material.to_c()
        self._check(self._b.material_insert(self._h, handle, C.byref(m)))

    def has_material(self, handle: int) -> bool:
        return bool(self._b.material_has(self._h, handle))

    def remove_material(self, handle: int):
        self._check(self._b.material_remove(self._h, handle))

    def insert_image(self, handle: int, rgba: np.ndarray, srgb: bool = True):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        assert rgba.ndim == 3 and rgba.shape[2] == 4
        self._check(self._b.image_insert_rgba8(self._h, handle, rgba.shape[1], rgba.shape[0], rgba.ctypes.data, 1 if srgb else 0))

    def remove_image(self, handle: int):
        self._check(self._b.image_remove(self._h, handle))

    def insert_instance(self, handle: int, instance: Instance):
        x = instance.xform12()
        self._check(self._b.instance_insert(self._h, handle, instance.mesh_handle, instance.material_handle, x.ctypes.data_as(C.POINTER(C.c_float))))

    def remove_instance(self, handle: int):
        self._check(self._b.instance_remove(self._h, handle))

    def insert_light(self, handle: int, light: Light):
        l = light.to_c()
        self._check(self._b.light_insert(self._h, handle, C.byref(l)))

    def remove_light(self, handle: int):
        self._check(self._b.light_remove(self._h, handle))

    def update_sun(self, sun: Sun):
        self._check(self._b.sun_update(self._h, sun.azimuth, sun.altitude))

    # --- cameras (lib.rs:252-297)
    def create_camera(self, camera: Camera) -> int:
        c = camera.to_c(); out = C.c_uint64()
        self._check(self._b.camera_create(self._h, C.byref(c), C.byref(out)))
        return out.value

    def update_camera(self, handle: int, camera: Camera):
        c = camera.to_c()
        self._check(self._b.camera_update(self._h, handle, C.byref(c)))

    def delete_camera(self, handle: int):
        self._check(self._b.camera_delete(self._h, handle))

    # --- seams
    def set_seed(self, seed: int):
        self._check(self._b.set_seed(self._h, seed))

    def set_blue_noise(self, rgba: np.ndarray):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        self._check(self._b.set_blue_noise(self._h, rgba.ctypes.data, rgba.nbytes))

    # --- read-back
    def buffer_stale(self, camera: int, buffer: Buffer) -> bool:
        """st_camera_buffer_stale: the camera's last frame (a lean frame) left this plane unwritten."""
        if not hasattr(self._b, "camera_buffer_stale"):
            return False
        out = C.c_int()
        self._check(self._b.camera_buffer_stale(self._h, camera, int(buffer), C.byref(out)))
        return out.value != 0

    def read_buffer(self, camera: int, buffer: Buffer, strict: bool = False) -> np.ndarray:
        """st_camera_read_buffer. strict=True refuses a plane the last frame did not write (the lean frame of the fast build,
        include/strolle_hip.h st_debug_keep_all_planes) instead of returning an earlier launch's content."""
        if strict and self.buffer_stale(camera, buffer):
            raise StrolleError(f"{Buffer(int(buffer)).name} was not written by the last frame (lean frame): keep_all_planes(True) stores every plane")
        n = C.c_size_t()
        self._check(self._b.camera_read_buffer(self._h, camera, int(buffer), None, 0, C.byref(n)))
        dtype = np.uint32 if int(buffer) == int(Buffer.DBG_USED_MEMORY) else np.float32
        out = np.empty(n.value // 4, dtype=dtype)
        self._check(self._b.camera_read_buffer(self._h, camera, int(buffer), out.ctypes.data, out.nbytes, C.byref(n)))
        return out

    def ray_count(self, camera: int, reset: bool = False) -> int:
        out = C.c_uint64()
        self._check(self._b.camera_ray_count(self._h, camera, C.byref(out), 1 if reset else 0))
        return out.value

    def read_scene(self, what: int) -> np.ndarray:
        n = C.c_size_t()
        self._check(self._b.debug_read_scene(self._h, what, None, 0, C.byref(n)))
        out = np.empty(n.value // 4, dtype=np.float32)
        if n.value:
            self._check(self._b.debug_read_scene(self._h, what, out.ctypes.data, out.nbytes, C.byref(n)))
        return out

    def read_lut(self, what: int) -> np.ndarray:
        """Atmosphere LUT (0 transmittance 256x64, 1 scattering 32x32, 2 sky 256x256) as [H, W, 4] float32."""
        n = C.c_size_t()
        self._check(self._b.debug_read_lut(self._h, what, None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        self._check(self._b.debug_read_lut(self._h, what, out.ctypes.data, out.size, C.byref(n)))
        w = (256, 32, 256)[what]
        return out.reshape(-1, w, 4)

    def world(self):
        lc, fr = C.c_uint32(), C.c_uint32()
        self._check(self._b.debug_world(self._h, C.byref(lc), C.byref(fr)))
        return lc.value, fr.value

    def set_bvh_refresh(self, refit):
        """st_set_bvh_refresh: False / 0 = rebuild on every change (the reference's behaviour), True / 1 = refit while instances only
        move, 2 = the same with the boxes recomputed on the device (ST_BVH_REFIT_DEVICE; libstrolle_hip.so only), 3 = the tree BUILT on the device
        straight into the wide stream while nothing observes the contract stream (ST_BVH_BUILD_DEVICE; libstrolle_hip.so only), 4 = the library's default
        (ST_BVH_AUTO: the first tree on the host — unless it hangs long leaf runs on large faces (auto_tree()), then the device builder's —, every later change as mode 3)."""
        refit = int(refit)
        if refit not in (0, 1, 2, 3, 4):
            raise StrolleError(f"unknown BVH refresh mode {refit}")
        if refit >= 2 and not hasattr(self._b, "debug_bvh_device_refits"):
            raise StrolleError("ST_BVH_REFIT_DEVICE is a mode of libstrolle_hip.so; this engine's library does not have it")
        self._check(self._b.set_bvh_refresh(self._h, refit))

    def bvh_device_refits(self) -> int:
        if not hasattr(self._b, "debug_bvh_device_refits"):
            raise StrolleError("bvh_device_refits() is a seam of libstrolle_hip.so (st_debug_bvh_device_refits); this engine's library does not export it")
        out = C.c_uint64()
        self._check(self._b.debug_bvh_device_refits(self._h, C.byref(out)))
        return out.value

    def device_builds(self) -> int:
        """ticks whose tree was built on the device so far (ST_BVH_BUILD_DEVICE)."""
        n = C.c_uint64()
        self._check(self._b.debug_device_builds(self._h, C.byref(n)))
        return int(n.value)

    def device_tree_refits(self) -> int:
        """ticks of ST_BVH_BUILD_DEVICE in which instances only moved and the device-built tree was refitted instead of rebuilt."""
        n = C.c_uint64()
        self._check(self._b.debug_device_tree_refits(self._h, C.byref(n)))
        return int(n.value)

    def device_bakes(self):
        """(launches of the device bake, triangles they baked) so far — StTuning::device_bake."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._b.debug_device_bakes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def bvh_refits(self):
        """(rebuilds, refits) so far."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._b.debug_bvh_refits(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def bvh_depth(self):
        """(longest chain of internal nodes in the uploaded BVH, traversal stack entries per ray)."""
        if not hasattr(self._b, "debug_bvh_depth"):
            raise StrolleError("bvh_depth() is a seam of libstrolle_hip.so (st_debug_bvh_depth); this engine's library does not export it")
        a, b = C.c_uint32(), C.c_uint32()
        self._check(self._b.debug_bvh_depth(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def walk_overflow(self):
        """(ticks that found a wide walk's overflow word set, entries the wide walks' stack holds now, 1 once the packet walk overflowed) — st_debug_walk_overflow."""
        n, entries, off = C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._check(self._b.debug_walk_overflow(self._h, C.byref(n), C.byref(entries), C.byref(off)))
        return n.value, entries.value, off.value

    def auto_tree(self):
        """(surface-area-weighted mean leaf-run length of the host's last tree, True when ST_BVH_AUTO gave this scene's first tree to the device builder) — st_debug_auto_tree."""
        w, d = C.c_float(), C.c_uint32()
        self._check(self._b.debug_auto_tree(self._h, C.byref(w), C.byref(d)))
        return float(w.value), bool(d.value)

    def image_rect(self, handle: int):
        """(x, y, w, h) of an image in the atlas, in texels."""
        r = (C.c_uint32 * 4)()
        self._check(self._b.debug_image_rect(self._h, handle, r))
        return tuple(r)

    def bvh_refresh(self):
        """(primitives in the tree, primitives that arrived inside subtrees reused from the previous tree)."""
        n, r = C.c_uint64(), C.c_uint64()
        self._check(self._b.debug_bvh_refresh(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value


_lib_cache = {}


def load_library(path: str = LIB_PATH) -> C.CDLL:
    if path not in _lib_cache:
        if not os.path.exists(path):
            raise StrolleError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        # One HIP runtime per process: PyTorch ships its own libamdhip64. If this library were loaded first it would bring
        # in /opt/rocm's copy, a later `import torch` would load its bundled one beside it, and device enumeration fails in
        # whichever comes second. So: a process that uses torch together with this package imports torch FIRST (tests and
        # bench.py do; then both share torch's runtime — this library only needs the HIP API). Nothing is imported behind
        # the caller's back unless STROLLE_HIP_PRELOAD_TORCH=1 asks for it.
        if os.environ.get("STROLLE_HIP_PRELOAD_TORCH") == "1" and "torch" not in sys.modules:
            import torch  # noqa: F401
        _lib_cache[path] = C.CDLL(path)
    return _lib_cache[path]


def library_build_commit(path: str = LIB_PATH) -> Optional[str]:
    """st_build_commit(): the commit compiled into the library that is loaded (None: a library older than round 6)."""
    lib = load_library(path)
    if not hasattr(lib, "st_build_commit"):
        return None
    lib.st_build_commit.restype = C.c_char_p
    return lib.st_build_commit().decode(errors="replace")


class Engine(EngineBase):
    """MI355X engine. device >= 0: HIP ordinal; device = -1: host-only (scene + BVH logic, no rendering)."""

    def __init__(self, device: int = 0, exact: Optional[bool] = None):
        """exact=None: the library default (fast arithmetic unless ST_EXACT=1 is set); True / False: st_engine_set_arithmetic."""
        super().__init__(_Binding(load_library(), "st_", True), device)
        if exact is not None:
            self.set_exact(exact)

    def set_exact(self, exact: bool):
        """st_engine_set_arithmetic: True = the bit-exact build of the kernels, False = the fast (default) build."""
        self._check(self._b.engine_set_arithmetic(self._h, 1 if exact else 0))

    @property
    def exact(self) -> bool:
        out = C.c_int()
        self._check(self._b.engine_get_arithmetic(self._h, C.byref(out)))
        return out.value == 1

    def write_buffer(self, camera: int, buffer: "Buffer", data: np.ndarray):
        """st_camera_write_buffer: the inverse of read_buffer (parity tests hand a launch its reference input planes)."""
        data = np.ascontiguousarray(data)
        self._check(self._b.camera_write_buffer(self._h, camera, int(buffer), data.ctypes.data, data.nbytes))

    def keep_all_planes(self, keep: bool):
        """st_debug_keep_all_planes: True = every frame stores every plane the reference does; False (default in the fast build) =
        the lean frame, which leaves planes nothing reads again unwritten (include/strolle_hip.h lists them)."""
        self._check(self._b.debug_keep_all_planes(self._h, 1 if keep else 0))

    def set_pass_mask(self, mask: int):
        """st_debug_set_pass_mask: bit set = that reference pass runs (PassBit)."""
        self._check(self._b.debug_set_pass_mask(self._h, mask & 0xFFFFFFFFFFFFFFFF))

    def set_launch_filter(self, mask: int):
        """st_debug_set_launch_filter: bit i set = the i-th launch of the frame's serial order is enqueued (measurement only)."""
        self._check(self._b.debug_set_launch_filter(self._h, mask & 0xFFFFFFFFFFFFFFFF))

    def last_launches(self):
        """Pass bits of every launch the last render_camera considered, in launch order."""
        arr = (C.c_uint64 * 64)(); n = C.c_size_t()
        self._check(self._b.debug_last_launches(self._h, arr, 64, C.byref(n)))
        return [arr[i] for i in range(min(n.value, 64))]

    def tick(self, stream: int = 0):
        self._check(self._b.tick(self._h, stream))

    def render_camera(self, handle: int, out_device_ptr: int = 0, stream: int = 0):
        """Enqueue CameraController::render; `out_device_ptr` = device address of a W*H RGBA32F buffer (0 = skip composition)."""
        self._check(self._b.render_camera(self._h, handle, out_device_ptr, stream))

    # ---- scene queries (include/strolle_hip.h "scene queries"): the scene of the last tick, enqueued on `stream`
    def trace_rays(self, rays_ptr: int, count: int, hits_ptr: int, coherent: bool = False, stream: int = 0, mapped_normal: bool = False):
        """st_scene_trace_rays: `count` StRay at device address `rays_ptr` -> StRayHit at `hits_ptr` (closest hits).
        coherent=True: ST_RAY_COHERENT (runs of 64 rays are camera-like; changes only speed).
        mapped_normal=True: ST_RAY_MAPPED_NORMAL (StRayHit.normal bent by the material's normal map, whatever the engine's switch says)."""
        flags = (RAY_COHERENT if coherent else 0) | (RAY_MAPPED_NORMAL if mapped_normal else 0)
        self._check(self._b.scene_trace_rays(self._h, rays_ptr, count, hits_ptr, flags, stream))

    def occluded(self, rays_ptr: int, count: int, out_ptr: int, stream: int = 0):
        """st_scene_occluded: one uint32 per ray at `out_ptr`, 1 where some triangle is hit at 0 < t < t_max."""
        self._check(self._b.scene_occluded(self._h, rays_ptr, count, out_ptr, stream))

    def pick(self, camera: int, pixels_ptr: int, count: int, hits_ptr: int, stream: int = 0):
        """st_camera_pick: `count` (x, y) uint32 pairs at `pixels_ptr` -> StRayHit at `hits_ptr`, through the camera as its last
        render saw it."""
        self._check(self._b.camera_pick(self._h, camera, pixels_ptr, count, hits_ptr, stream))

    def render_aovs(self, camera: int, planes: dict, stream=None):
        """st_camera_render_aovs: {Aov: device address or torch tensor} -> the camera's per-pixel AOVs of the frame on screen, enqueued on
        `stream` (a HIP stream handle, a torch stream, or None = the null stream). Planes are width x height elements, row-major;
        aov_planes() allocates them. Only the camera's window is written."""
        t = StAovTargets(); t.struct_size = C.sizeof(StAovTargets)
        for k, v in planes.items():
            k = Aov(k)
            if v is None:
                continue
            if hasattr(v, "data_ptr"):
                scalar, comps = AOV_ELEMENT[k]
                per_pixel = v.shape[-1] if comps > 1 and v.dim() > 0 else comps
                if not v.is_contiguous() or v.element_size() != np.dtype(scalar).itemsize or per_pixel != comps:
                    raise StrolleError(f"AOV plane {k.name}: expected a contiguous tensor of {comps} x {np.dtype(scalar).name} per pixel")
                v = v.data_ptr()
            t.planes[int(k)] = int(v)
        if stream is not None and hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        self._check(self._b.camera_render_aovs(self._h, camera, C.byref(t), stream or 0))

    def set_pose(self, instance: int, matrices):
        """st_instance_set_pose: matrices (J, 3, 4) like Instance.transform — joint transform x inverse bind matrix, into the instance's
        object space; applied at the next tick. None = back to the bind pose."""
        if matrices is None:
            self._check(self._b.instance_set_pose(self._h, instance, None, 0)); return
        m = np.asarray(matrices, np.float32).reshape(-1, 3, 4)
        flat = np.ascontiguousarray(m.transpose(0, 2, 1).reshape(-1), dtype=np.float32)   # per joint: columns x, y, z, t
        self._check(self._b.instance_set_pose(self._h, instance, flat.ctypes.data_as(C.POINTER(C.c_float)), len(m)))

    def set_morph_weights(self, instance: int, weights):
        """st_instance_set_morph_weights: one weight per target of the instance's mesh, applied at the next tick. None = back to the base shape."""
        if weights is None:
            self._check(self._b.instance_set_morph_weights(self._h, instance, None, 0)); return
        w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
        self._check(self._b.instance_set_morph_weights(self._h, instance, w.ctypes.data_as(C.POINTER(C.c_float)), len(w)))

    def morphing_stats(self):
        """st_debug_morphing: (ticks that ran a morph stage, triangles morphed, bytes of deltas the device store holds)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._b.debug_morphing(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def skinning_stats(self):
        """st_debug_skinning: (skin launches, triangles skinned, batched host read-backs of posed triangles)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._b.debug_skinning(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def read_posed(self, instance: int) -> np.ndarray:
        """st_debug_read_posed: the instance's posed object-space triangles as the device holds them, (n, 24) float32 (positions 9,
        normals 9, uvs 6)."""
        n = C.c_size_t()
        self._check(self._b.debug_read_posed(self._h, instance, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        self._check(self._b.debug_read_posed(self._h, instance, out.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)))
        return out.reshape(-1, 24)

    # ---- deformation motion (include/strolle_hip.h "skinned meshes"): takes effect at the next tick
    def set_deformation_motion(self, enabled: bool):
        """st_engine_set_deformation_motion: the velocity plane, reprojection and the MOTION AOV follow skinned deformations too."""
        self._check(self._b.engine_set_deformation_motion(self._h, 1 if enabled else 0))

    @property
    def deformation_motion(self) -> bool:
        """st_engine_get_deformation_motion."""
        on = C.c_int()
        self._check(self._b.engine_get_deformation_motion(self._h, C.byref(on)))
        return bool(on.value)

    # ---- normal mapping (include/strolle_hip.h "normal mapping"): takes effect with the next render, AOV, pick or query call
    def set_normal_mapping(self, enabled: bool):
        """st_engine_set_normal_mapping: primary hits, the NORMAL AOV and picks take the normal bent by the material's normal map."""
        self._check(self._b.engine_set_normal_mapping(self._h, 1 if enabled else 0))

    def get_normal_mapping(self) -> bool:
        """st_engine_get_normal_mapping."""
        on = C.c_int()
        self._check(self._b.engine_get_normal_mapping(self._h, C.byref(on)))
        return bool(on.value)

    def deformation_stats(self):
        """st_debug_deformation: (instances the last tick left a previous pose, bytes of device memory their second regions hold)."""
        n, b = C.c_uint64(), C.c_uint64()
        self._check(self._b.debug_deformation(self._h, C.byref(n), C.byref(b)))
        return n.value, b.value

    # ---- the output chain's settings: every st_camera_set_<stage> takes a descriptor or null, every st_camera_get_<stage> returns (descriptor, on)
    def _set_stage(self, setter, make_desc, camera: int, desc, kw):
        """a descriptor, or make_desc(**kw) when keywords are given; neither = off"""
        if desc is None and kw:
            desc = make_desc(**kw)
        self._check(setter(self._h, camera, C.byref(desc) if desc is not None else None))

    def _get_stage(self, getter, desc_type, camera: int):
        d, on = desc_type(), C.c_int()
        self._check(getter(self._h, camera, C.byref(d), C.byref(on)))
        return d, bool(on.value)

    # ---- display transforms (include/strolle_hip.h "display transforms"): take effect at the camera's next render
    def set_display(self, camera: int, desc: Optional[StDisplayDesc] = None, **kw):
        """st_camera_set_display: a StDisplayDesc, or display_desc(**kw) when keywords are given; neither = off (the output as without a display)."""
        self._set_stage(self._b.camera_set_display, display_desc, camera, desc, kw)

    def display(self, camera: int):
        """st_camera_get_display: (the last StDisplayDesc set, whether the display is on)."""
        return self._get_stage(self._b.camera_get_display, StDisplayDesc, camera)

    def exposure(self, camera: int):
        """st_camera_exposure (blocking): (scale the next frame uses, metered EV, adapted EV) as the device holds them."""
        s, m, a = C.c_float(), C.c_float(), C.c_float()
        self._check(self._b.camera_exposure(self._h, camera, C.byref(s), C.byref(m), C.byref(a)))
        return s.value, m.value, a.value

    def camera_histogram(self, camera: int) -> np.ndarray:
        """st_debug_camera_histogram (blocking): the 64 bins metered from the camera's last auto-exposure frame."""
        out = np.zeros(DISPLAY_BINS, np.uint32)
        self._check(self._b.debug_camera_histogram(self._h, camera, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    # ---- output post-processing (include/strolle_hip.h "post-processing"): takes effect at the camera's next render
    def set_post(self, camera: int, desc: Optional[StPostDesc] = None, **kw):
        """st_camera_set_post: a StPostDesc, or post_desc(**kw) when keywords are given; neither = off."""
        self._set_stage(self._b.camera_set_post, post_desc, camera, desc, kw)

    def post(self, camera: int):
        """st_camera_get_post: (the last StPostDesc set, whether post-processing is on)."""
        return self._get_stage(self._b.camera_get_post, StPostDesc, camera)

    def output_size(self, camera: int):
        """st_camera_output_size: (width, height) of the buffer st_render_camera writes."""
        w, h = C.c_uint32(), C.c_uint32()
        self._check(self._b.camera_output_size(self._h, camera, C.byref(w), C.byref(h)))
        return w.value, h.value

    def post_process(self, desc: StPostDesc, src_ptr: int, width: int, height: int, dst_ptr: int, dst_format: int = 0, stream: int = 0):
        """st_post_process: FXAA and / or resampling of any RGBA32F device image into dst (the desc's output size) in dst_format."""
        self._check(self._b.post_process(self._h, C.byref(desc), src_ptr, width, height, dst_ptr, int(dst_format), stream))

    # ---- the upscale stage (include/strolle_hip.h "upscaling"): takes effect at the camera's next render
    def set_upscale(self, camera: int, desc: Optional[StUpscaleDesc] = None, **kw):
        """st_camera_set_upscale: a StUpscaleDesc, or upscale_desc(**kw) when keywords are given; neither = off."""
        self._set_stage(self._b.camera_set_upscale, upscale_desc, camera, desc, kw)

    def upscale(self, camera: int):
        """st_camera_get_upscale: (the last StUpscaleDesc set, whether the stage is on)."""
        return self._get_stage(self._b.camera_get_upscale, StUpscaleDesc, camera)

    def set_upscale_fused(self, tile: int):
        """st_debug_set_upscale_fused: 0 = the two steps as two launches, 1 / 2 / 3 = one launch over 64 x 8 / 32 x 32 / 64 x 16 output tiles."""
        self._check(self._b.debug_set_upscale_fused(self._h, int(tile)))

    def upscale_process(self, desc: StUpscaleDesc, src_ptr: int, width: int, height: int, dst_ptr: int, dst_format: int = 0, stream: int = 0):
        """st_upscale_process: upscaling and / or sharpening of any RGBA32F device image into dst (the desc's output size) in dst_format."""
        self._check(self._b.upscale_process(self._h, C.byref(desc), src_ptr, width, height, dst_ptr, int(dst_format), stream))

    # ---- bloom (include/strolle_hip.h "bloom"): takes effect at the camera's next render
    def set_bloom(self, camera: int, desc: Optional[StBloomDesc] = None, **kw):
        """st_camera_set_bloom: a StBloomDesc, or bloom_desc(**kw) when keywords are given; neither = off."""
        self._set_stage(self._b.camera_set_bloom, bloom_desc, camera, desc, kw)

    def bloom(self, camera: int):
        """st_camera_get_bloom: (the last StBloomDesc set, whether bloom is on)."""
        return self._get_stage(self._b.camera_get_bloom, StBloomDesc, camera)

    def bloom_plan(self, desc: StBloomDesc, width: int, height: int):
        """st_bloom_plan (host arithmetic): (levels, [(width, height) per mip], float32 blend factors per level)."""
        n, sizes, factors = C.c_uint32(), (C.c_uint32 * 16)(), (C.c_float * 8)()
        self._check(self._b.bloom_plan(C.byref(desc), width, height, C.byref(n), sizes, factors))
        return n.value, [(sizes[2 * k], sizes[2 * k + 1]) for k in range(n.value)], np.array(factors[:n.value], np.float32)

    def bloom_process(self, desc: StBloomDesc, src_ptr: int, width: int, height: int, dst_ptr: int, dst_format: int = 0,
                      display: Optional[StDisplayDesc] = None, stream: int = 0):
        """st_bloom_process: bloom over any RGBA32F device image, then the (manual) display transform, into dst (width x height) in dst_format."""
        self._check(self._b.bloom_process(self._h, C.byref(desc), C.byref(display) if display is not None else None, src_ptr, width, height,
                                          dst_ptr, int(dst_format), stream))

    def set_bloom_tail(self, lds_bytes: int = -1) -> int:
        """st_debug_set_bloom_tail: the LDS budget of the bloom chain's fused tail (-1 the device's, 0 no tail); returns the bytes in force."""
        out = C.c_uint32()
        self._check(self._b.debug_set_bloom_tail(self._h, int(lds_bytes), C.byref(out)))
        return out.value

    # ---- motion blur (include/strolle_hip.h "motion blur"): takes effect at the camera's next render
    def set_motion_blur(self, camera: int, desc: Optional[StMotionBlurDesc] = None, **kw):
        """st_camera_set_motion_blur: a StMotionBlurDesc, or motion_blur_desc(**kw) when keywords are given; neither = off."""
        self._set_stage(self._b.camera_set_motion_blur, motion_blur_desc, camera, desc, kw)

    def get_motion_blur(self, camera: int):
        """st_camera_get_motion_blur: (the last StMotionBlurDesc set, whether the blur is on)."""
        return self._get_stage(self._b.camera_get_motion_blur, StMotionBlurDesc, camera)

    def motion_blur_process(self, desc: StMotionBlurDesc, color_ptr: int, velocity_ptr: int, depth_ptr: int, width: int, height: int, dst_ptr: int,
                            dst_format: int = 0, display: Optional[StDisplayDesc] = None, stream: int = 0):
        """st_motion_blur_process: the blur over any RGBA32F colour, f32x2 velocity and f32 depth device planes, then the (manual) display
        transform, into dst (width x height) in dst_format."""
        self._check(self._b.motion_blur_process(self._h, C.byref(desc), C.byref(display) if display is not None else None, color_ptr, velocity_ptr,
                                                depth_ptr, width, height, dst_ptr, int(dst_format), stream))

    # ---- depth of field (include/strolle_hip.h "depth of field"): takes effect at the camera's next render
    def set_dof(self, camera: int, desc: Optional[StDofDesc] = None, **kw):
        """st_camera_set_dof: a StDofDesc, or dof_desc(**kw) when keywords are given; neither = off."""
        self._set_stage(self._b.camera_set_dof, dof_desc, camera, desc, kw)

    def get_dof(self, camera: int):
        """st_camera_get_dof: (the last StDofDesc set, whether depth of field is on)."""
        return self._get_stage(self._b.camera_get_dof, StDofDesc, camera)

    def dof_process(self, desc: StDofDesc, projection, color_ptr: int, depth_ptr: int, width: int, height: int, dst_ptr: int, dst_format: int = 0,
                    display: Optional[StDisplayDesc] = None, stream: int = 0):
        """st_dof_process: depth of field over any RGBA32F colour and f32 depth device planes rendered with `projection` (16 floats, column
        major), then the (manual) display transform, into dst (width x height) in dst_format."""
        proj = (C.c_float * 16)(*[float(v) for v in projection])
        self._check(self._b.dof_process(self._h, C.byref(desc), C.byref(display) if display is not None else None, proj, color_ptr, depth_ptr, width, height,
                                        dst_ptr, int(dst_format), stream))

    # ---- fog (include/strolle_hip.h "fog"): takes effect at the camera's next render
    def set_fog(self, camera: int, desc: Optional[StFogDesc] = None, **kw):
        """st_camera_set_fog: a StFogDesc, or fog_desc(**kw) when keywords are given; neither = off."""
        self._set_stage(self._b.camera_set_fog, fog_desc, camera, desc, kw)

    def get_fog(self, camera: int):
        """st_camera_get_fog: (the last StFogDesc set, whether fog is on)."""
        return self._get_stage(self._b.camera_get_fog, StFogDesc, camera)

    def fog_process(self, desc: StFogDesc, transform, projection, color_ptr: int, depth_ptr: int, width: int, height: int, dst_ptr: int, dst_format: int = 0,
                    display: Optional[StDisplayDesc] = None, stream: int = 0):
        """st_fog_process: fog over any RGBA32F colour and f32 depth device planes rendered with `transform` and `projection` (16 floats
        each, column major), then the (manual) display transform, into dst (width x height) in dst_format."""
        xf, proj = (C.c_float * 16)(*[float(v) for v in transform]), (C.c_float * 16)(*[float(v) for v in projection])
        self._check(self._b.fog_process(self._h, C.byref(desc), C.byref(display) if display is not None else None, xf, proj, color_ptr, depth_ptr, width, height,
                                        dst_ptr, int(dst_format), stream))

    # ---- lens effects (include/strolle_hip.h "lens effects"): takes effect at the camera's next render
    def set_lens(self, camera: int, desc: Optional[StLensDesc] = None, **kw):
        """st_camera_set_lens: a StLensDesc, or lens_desc(**kw) when keywords are given; neither = off."""
        self._set_stage(self._b.camera_set_lens, lens_desc, camera, desc, kw)

    def get_lens(self, camera: int):
        """st_camera_get_lens: (the last StLensDesc set, whether the node is on)."""
        return self._get_stage(self._b.camera_get_lens, StLensDesc, camera)

    def lens_plan(self, desc: StLensDesc, width: int, height: int) -> StLensPlan:
        """st_lens_plan (the module's lens_plan)."""
        return lens_plan(desc, width, height)

    def lens_process(self, desc: StLensDesc, src_ptr: int, width: int, height: int, dst_ptr: int, dst_format: int = 0, display: Optional[StDisplayDesc] = None,
                     stream: int = 0):
        """st_lens_process: the node's launch over any RGBA32F device plane, through the (manual) display transform, into dst (width x
        height) in dst_format."""
        self._check(self._b.lens_process(self._h, C.byref(desc), C.byref(display) if display is not None else None, src_ptr, width, height, dst_ptr, int(dst_format), stream))

    def set_lens_gather(self, force: bool):
        """st_debug_set_lens_gather: descriptors without taps run the gather instantiation (measurement and tests)."""
        self._check(self._b.debug_set_lens_gather(self._h, 1 if force else 0))

    # ---- colour grading (include/strolle_hip.h "colour grading"): takes effect at the camera's next render; tables at the next tick
    def set_color_grading(self, camera: int, desc: Optional[StColorGradingDesc] = None, **kw):
        """st_camera_set_color_grading: a StColorGradingDesc, or color_grading_desc(**kw) when keywords are given; neither = off."""
        self._set_stage(self._b.camera_set_color_grading, color_grading_desc, camera, desc, kw)

    def get_color_grading(self, camera: int):
        """st_camera_get_color_grading: (the last StColorGradingDesc set, whether the node is on)."""
        return self._get_stage(self._b.camera_get_color_grading, StColorGradingDesc, camera)

    def insert_lut(self, handle: int, rgb):
        """st_lut_insert: an (N, N, N, 3) float32 table indexed [b, g, r] (red fastest, a .cube file's order; load_cube returns it so)."""
        t = np.ascontiguousarray(rgb, np.float32)
        if t.ndim != 4 or t.shape[3] != 3 or not (t.shape[0] == t.shape[1] == t.shape[2]):
            raise StrolleError("LUT: expected an (N, N, N, 3) array")
        self._check(self._b.lut_insert(self._h, handle, t.shape[0], t.ctypes.data_as(C.POINTER(C.c_float))))

    def remove_lut(self, handle: int):
        self._check(self._b.lut_remove(self._h, handle))

    def color_grading_plan(self, desc: StColorGradingDesc):
        """st_color_grading_plan (the module's color_grading_plan)."""
        return color_grading_plan(desc)

    def color_grading_process(self, desc: StColorGradingDesc, src_ptr: int, width: int, height: int, dst_ptr: int, dst_format: int = 0,
                              display: Optional[StDisplayDesc] = None, lut_ptr: int = 0, lut_size: int = 0, stream: int = 0):
        """st_color_grading_process: the node's launch over any RGBA32F device plane, with the (manual) display transform between its two
        halves, into dst (width x height) in dst_format. lut_ptr: lut_size^3 float4 in device memory, or 0 for no LUT step."""
        self._check(self._b.color_grading_process(self._h, C.byref(desc), C.byref(display) if display is not None else None, lut_ptr or None, lut_size, src_ptr, width,
                                                  height, dst_ptr, int(dst_format), stream))

    # ---- light shafts (include/strolle_hip.h "light shafts"): takes effect at the camera's next render
    def set_light_shafts(self, camera: int, desc: Optional[StLightShaftsDesc] = None, **kw):
        """st_camera_set_light_shafts: a StLightShaftsDesc, or light_shafts_desc(**kw) when keywords are given; neither = off."""
        self._set_stage(self._b.camera_set_light_shafts, light_shafts_desc, camera, desc, kw)

    def get_light_shafts(self, camera: int):
        """st_camera_get_light_shafts: (the last StLightShaftsDesc set, whether the node is on)."""
        return self._get_stage(self._b.camera_get_light_shafts, StLightShaftsDesc, camera)

    def light_shafts_process(self, desc: StLightShaftsDesc, transform, projection, color_ptr: int, depth_ptr: int, width: int, height: int, dst_ptr: int,
                             dst_format: int = 0, display: Optional[StDisplayDesc] = None, stream: int = 0):
        """st_light_shafts_process: shafts through the engine's live scene (after a tick) over any RGBA32F colour and f32 depth device planes
        rendered with `transform` and `projection` (16 floats each, column major), then the (manual) display transform, into dst."""
        xf, proj = (C.c_float * 16)(*[float(v) for v in transform]), (C.c_float * 16)(*[float(v) for v in projection])
        self._check(self._b.light_shafts_process(self._h, C.byref(desc), C.byref(display) if display is not None else None, xf, proj, color_ptr, depth_ptr,
                                                 width, height, dst_ptr, int(dst_format), stream))

    # ---- environment lighting (include/strolle_hip.h "environment lighting"): takes effect at the next tick
    def set_environment(self, texels, intensity: float = 1.0, yaw: float = 0.0, keep_sun: bool = False, uniform: bool = False):
        """st_environment_set / st_environment_set_device: an equirectangular map, (H, W, 3 or 4) float32, row 0 the zenith, the centre looking
        down -Z. A numpy array is copied by the call; a CUDA tensor is read by the next tick (keep it alive and unchanged until then)."""
        desc = environment_desc(intensity, yaw, keep_sun, uniform)
        if hasattr(texels, "data_ptr") and getattr(texels, "is_cuda", False):
            if texels.dim() != 3 or texels.element_size() != 4 or not texels.is_floating_point():
                raise StrolleError("environment map: expected an (H, W, 3 or 4) float32 tensor")
            h, w, ch = texels.shape
            pitch = texels.stride(0) * 4
            if texels.stride(2) != 1 or texels.stride(1) != ch:
                raise StrolleError("environment map: rows must be contiguous")
            self._check(self._b.environment_set_device(self._h, texels.data_ptr(), w, h, ch, pitch, C.byref(desc)))
            return
        a = np.ascontiguousarray(texels, dtype=np.float32)
        if a.ndim != 3:
            raise StrolleError("environment map: expected an (H, W, 3 or 4) array")
        h, w, ch = a.shape
        self._check(self._b.environment_set(self._h, a.ctypes.data, w, h, ch, C.byref(desc)))

    def update_environment(self, intensity: float = 1.0, yaw: float = 0.0, keep_sun: bool = False, uniform: bool = False):
        """st_environment_update: intensity, yaw and flags of the map, without re-uploading it."""
        self._check(self._b.environment_update(self._h, C.byref(environment_desc(intensity, yaw, keep_sun, uniform))))

    def clear_environment(self):
        """st_environment_clear: back to the atmosphere at the next tick."""
        self._check(self._b.environment_clear(self._h))

    def _env_seam(self, fn, inp, n, out_cols):
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        x = torch.as_tensor(np.ascontiguousarray(inp, np.float32), device=dev).contiguous()
        out = torch.zeros((n, out_cols), dtype=torch.float32, device=dev)
        self._check(fn(self._h, x.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def environment_eval(self, dirs) -> np.ndarray:
        """st_debug_environment_eval: (n, 3) world directions -> (n, 3) radiance of the live map."""
        d = np.asarray(dirs, np.float32).reshape(-1, 3)
        return self._env_seam(self._b.debug_environment_eval, d, len(d), 3)

    def environment_sample(self, u) -> np.ndarray:
        """st_debug_environment_sample: (n, 3) uniforms in [0, 1) -> (n, 4) (direction xyz, solid-angle pdf): the first picks the cell,
        the other two place the direction across and down it."""
        u = np.asarray(u, np.float32).reshape(-1, 3)
        return self._env_seam(self._b.debug_environment_sample, u, len(u), 4)

    def environment_pdf(self, dirs) -> np.ndarray:
        """st_debug_environment_pdf: (n, 3) world directions -> (n,) solid-angle pdf of the importance sampler."""
        d = np.asarray(dirs, np.float32).reshape(-1, 3)
        return self._env_seam(self._b.debug_environment_pdf, d, len(d), 1)[:, 0]

    def environment_table(self) -> np.ndarray:
        """st_debug_environment_table: the live map's importance table, (cells_y, cells_x) of ENV_CELL_DTYPE."""
        gx, gy = C.c_uint32(), C.c_uint32()
        self._check(self._b.debug_environment_table(self._h, None, 0, C.byref(gx), C.byref(gy)))
        out = np.zeros((gy.value, gx.value), ENV_CELL_DTYPE)
        self._check(self._b.debug_environment_table(self._h, out.ctypes.data, out.nbytes, C.byref(gx), C.byref(gy)))
        return out

    def environment_sanitized(self) -> int:
        """st_debug_environment_sanitized: texels the device uploads set to 0 (NaN, infinite or negative channels)."""
        n = C.c_uint64()
        self._check(self._b.debug_environment_sanitized(self._h, C.byref(n)))
        return n.value

    def trace_rays_host(self, rays: np.ndarray) -> np.ndarray:
        """st_scene_trace_rays_host: a RAY_DTYPE array in host memory -> a HIT_DTYPE array (blocking)."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        self._check(self._b.scene_trace_rays_host(self._h, rays.ctypes.data, rays.shape[0], hits.ctypes.data))
        return hits

    def set_output_format(self, handle: int, fmt: "OutputFormat"):
        """viewport.format (camera.rs:170-175): what st_render_camera writes into its output buffer."""
        self._check(self._b.camera_set_output_format(self._h, handle, int(fmt)))

    def present_copy(self, handle: int, src_device_ptr: int, dst_host_ptr: int, nbytes: int, stream: int = 0):
        """st_camera_present_copy: the frame just composed into `src_device_ptr` on `stream` -> page-locked host memory,
        asynchronously on the camera's copy stream (the facade's present path; the next frame overlaps the copy)."""
        self._check(self._b.camera_present_copy(self._h, handle, src_device_ptr, dst_host_ptr, nbytes, stream))

    def present_ready(self, handle: int, dst_host_ptr: int, wait: bool = False) -> bool:
        """st_camera_present_ready: has the copy into `dst_host_ptr` landed? wait=True blocks until it has."""
        out = C.c_int()
        self._check(self._b.camera_present_ready(self._h, handle, dst_host_ptr, 1 if wait else 0, C.byref(out)))
        return out.value == 1

    def set_camera_rows(self, handle: int, y0: int, y1: int):
        self._check(self._b.camera_set_rows(self._h, handle, y0, y1))

    def variance_flags(self, cam: int) -> np.ndarray:
        """st_debug_variance_flags: one uint64 per 8x8 tile, bit = pixel whose variance estimate takes the short-history branch."""
        n = C.c_size_t()
        self._check(self._b.debug_variance_flags(self._h, cam, None, 0, C.byref(n)))
        mask = np.zeros(n.value, np.uint64)
        self._check(self._b.debug_variance_flags(self._h, cam, mask.ctypes.data, mask.size, C.byref(n)))
        return mask

    def set_camera_window(self, handle: int, x0: int, y0: int, x1: int, y1: int):
        """st_camera_set_window: restrict the camera's launches to [x0, x1) x [y0, y1) of the viewport (0, 0 = everything on that axis)."""
        self._check(self._b.camera_set_window(self._h, handle, x0, y0, x1, y1))

    # ---- multi-GPU behind the boundary (include/strolle_hip.h st_dist_*)
    def dist_init(self, rank: int, world: int, unique_id: bytes):
        """RCCL transport: `unique_id` = dist_unique_id() of rank 0, handed to every rank by the caller's own means."""
        if not isinstance(unique_id, (bytes, bytearray)) or len(unique_id) != 128:   # a truncated id would hang every rank in ncclCommInitRank
            raise StrolleError(f"dist_init: the RCCL unique id has 128 bytes, got {len(unique_id) if hasattr(unique_id, '__len__') else type(unique_id).__name__}")
        uid = StDistUniqueId(); C.memmove(C.byref(uid), bytes(unique_id), 128)
        self._check(self._b.dist_init(self._h, rank, world, C.byref(uid)))

    def dist_init_local(self, rank: int, world: int, group: int = 1):
        """In-process transport: the engines of this process that share `group` (tests, single-GPU boxes)."""
        self._check(self._b.dist_init_local(self._h, rank, world, group))

    def dist_shutdown(self):
        self._check(self._b.dist_shutdown(self._h))

    def dist_set_partition(self, cam: int, cols: int = 0, apron: int = 0):
        """This rank's tile of the camera's frame (+ apron) becomes the camera's window. Returns (owned, window) as (x0, y0, x1, y1)."""
        o, w = StDistRect(), StDistRect()
        self._check(self._b.dist_set_partition(self._h, cam, cols, apron, C.byref(o), C.byref(w)))
        return o.as_tuple(), w.as_tuple()

    def dist_set_grid(self, cam: int, grid: "StDistGrid", apron: int = 0):
        """st_dist_set_grid: like dist_set_partition with the tiles of `grid` (dist_grid / dist_grid_rebalance); every rank sets the same grid."""
        o, w = StDistRect(), StDistRect()
        self._check(self._b.dist_set_grid(self._h, cam, C.byref(grid), apron, C.byref(o), C.byref(w)))
        return o.as_tuple(), w.as_tuple()

    def dist_gather(self, cam: int, frame_ptr: int, full_ptr: int = 0, stream: int = 0):
        """st_dist_gather: this rank's tile of `frame_ptr` travels to rank 0, which assembles the frame at `full_ptr`."""
        self._check(self._b.dist_gather(self._h, cam, frame_ptr, full_ptr or None, stream))

    def dist_wait(self, cam: int, frame_ptr: int = 0, stream: int = 0, host: bool = True):
        """st_dist_wait: behind the gather that read `frame_ptr` (0: every gather in flight); host=True blocks the caller."""
        self._check(self._b.dist_wait(self._h, cam, frame_ptr or None, stream, 1 if host else 0))

    def dist_gather_ms(self, cam: int) -> float:
        out = C.c_float()
        self._check(self._b.dist_gather_ms(self._h, cam, C.byref(out)))
        return out.value

    def insert_device_image(self, handle: int, device_ptr: int, width: int, height: int, row_pitch_bytes: int = 0, dynamic: bool = False):
        """ImageData::Texture: RGBA8 pixels in device memory (e.g. `tensor.data_ptr()` of a [h, w, 4] uint8 CUDA tensor)."""
        self._check(self._b.image_insert_device_rgba8(self._h, handle, width, height, device_ptr, row_pitch_bytes or width * 4, 1 if dynamic else 0))

    def load_gltf(self, source, base_dir: Optional[str] = None, first_handle: int = 1, first_image_handle: int = 1000,
                  reflectance: Optional[float] = None, perceptual_roughness: Optional[float] = None, subdivide: int = 0, light_radius: float = 0.0) -> dict:
        """st_scene_load_gltf: `source` is a path to a .gltf / .glb file, or the file's bytes (external buffers and images
        are then read relative to `base_dir`). Returns the loader's summary."""
        opt = StGltfOptions(first_handle, first_image_handle, 0, 0.0, 0.0, subdivide, light_radius, 0)
        if reflectance is not None:
            opt.override_mask |= 1; opt.reflectance = reflectance
        if perceptual_roughness is not None:
            opt.override_mask |= 2; opt.perceptual_roughness = perceptual_roughness
        out = StGltfSummary()
        if isinstance(source, (bytes, bytearray, memoryview)):
            data = bytes(source)
            self._check(self._b.scene_load_gltf_memory(self._h, data, len(data), base_dir.encode() if base_dir else None, C.byref(opt), C.byref(out)))
        else:
            self._check(self._b.scene_load_gltf(self._h, os.fsencode(source), C.byref(opt), C.byref(out)))
        return {name: getattr(out, name) for name, _ in StGltfSummary._fields_}

    def tuning(self) -> "StTuning":
        """st_engine_get_tuning: the engine's scheduling / tuning switches (a copy; change fields and hand it to set_tuning)."""
        t = StTuning()
        self._check(self._b.engine_get_tuning(self._h, C.byref(t)))
        return t

    def set_tuning(self, tuning=None, **fields):
        """st_engine_set_tuning. Either a whole StTuning, or keyword fields applied on top of the current one: set_tuning(fuse=0)."""
        t = tuning if tuning is not None else self.tuning()
        for k, v in fields.items():
            if not hasattr(t, k):
                raise StrolleError(f"StTuning has no field {k!r}")
            setattr(t, k, int(v))
        self._check(self._b.engine_set_tuning(self._h, C.byref(t)))

    def copy_bandwidth(self, nbytes: int = 1 << 30, iters: int = 6) -> float:
        """st_debug_copy_bandwidth: GB/s (read + write) of the library's own grid-stride float4 copy on this device."""
        out = C.c_double()
        self._check(self._b.debug_copy_bandwidth(self._h, nbytes, iters, C.byref(out)))
        return out.value

    def profile_enable(self, flags):
        """st_profile_enable: bit 0 = per-kernel event timing (serial execution), bit 1 = traversal-byte counters; True = 1."""
        self._check(self._b.profile_enable(self._h, int(flags)))

    def profile_read(self, reset: bool = True):
        arr = (StKernelProfile * PROFILE_MAX_KERNELS)(); n = C.c_size_t()
        self._check(self._b.profile_read(self._h, arr, PROFILE_MAX_KERNELS, C.byref(n), 1 if reset else 0))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms, algorithmic_bytes=arr[i].algorithmic_bytes, traversal_bytes=arr[i].traversal_bytes)
                for i in range(n.value)]


def dist_partition(width: int, height: int, world: int, rank: int, cols: int = 0):
    """st_dist_partition: the tile (x0, y0, x1, y1) rank `rank` of `world` owns (cols = 0: the default grid)."""
    lib = load_library()
    r = StDistRect()
    lib.st_dist_partition.restype = C.c_int
    lib.st_dist_partition.argtypes = [C.c_uint32] * 5 + [C.POINTER(StDistRect)]
    if lib.st_dist_partition(width, height, world, cols, rank, C.byref(r)) != 0:
        lib.st_last_error.restype = C.c_char_p
        raise StrolleError(lib.st_last_error().decode(errors="replace"))
    return r.as_tuple()


def _dist_call(name, argtypes, *args):
    lib = load_library()
    f = getattr(lib, name)
    f.restype = C.c_int; f.argtypes = argtypes
    if f(*args) != 0:
        lib.st_last_error.restype = C.c_char_p
        raise StrolleError(lib.st_last_error().decode(errors="replace"))


def dist_grid(width: int, height: int, world: int, cols: int = 0) -> StDistGrid:
    """st_dist_grid: the equal split as a grid (its tiles are st_dist_partition's)."""
    g = StDistGrid()
    _dist_call("st_dist_grid", [C.c_uint32] * 4 + [C.POINTER(StDistGrid)], width, height, world, cols, C.byref(g))
    return g


def dist_grid_tile(grid: StDistGrid, rank: int):
    r = StDistRect()
    _dist_call("st_dist_grid_tile", [C.POINTER(StDistGrid), C.c_uint32, C.POINTER(StDistRect)], C.byref(grid), rank, C.byref(r))
    return r.as_tuple()


def dist_grid_rebalance(width: int, height: int, grid: StDistGrid, tile_cost, max_step: int = 0) -> StDistGrid:
    """st_dist_grid_rebalance: the grid whose rows, then each row's tiles, would cost the same, from one cost per tile in rank order."""
    cost = (C.c_float * (grid.cols * grid.rows))(*[float(v) for v in tile_cost])
    out = StDistGrid()
    _dist_call("st_dist_grid_rebalance", [C.c_uint32, C.c_uint32, C.POINTER(StDistGrid), C.POINTER(C.c_float), C.c_uint32, C.POINTER(StDistGrid)],
               width, height, C.byref(grid), cost, max_step, C.byref(out))
    return out


def dist_window(width: int, height: int, owned, apron: int):
    """st_dist_window: `owned` widened by `apron` pixels towards its neighbours, on the 16 x 8 pixel grid."""
    lib = load_library()
    o, w = StDistRect(*owned), StDistRect()
    lib.st_dist_window.restype = C.c_int
    lib.st_dist_window.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(StDistRect), C.c_uint32, C.POINTER(StDistRect)]
    if lib.st_dist_window(width, height, C.byref(o), apron, C.byref(w)) != 0:
        lib.st_last_error.restype = C.c_char_p
        raise StrolleError(lib.st_last_error().decode(errors="replace"))
    return w.as_tuple()


def dist_unique_id() -> bytes:
    """st_dist_unique_id (ncclGetUniqueId): rank 0 makes it, every rank passes it to Engine.dist_init."""
    lib = load_library()
    uid = StDistUniqueId()
    lib.st_dist_unique_id.restype = C.c_int
    lib.st_dist_unique_id.argtypes = [C.POINTER(StDistUniqueId)]
    if lib.st_dist_unique_id(C.byref(uid)) != 0:
        lib.st_last_error.restype = C.c_char_p
        raise StrolleError(lib.st_last_error().decode(errors="replace"))
    return bytes(C.string_at(C.byref(uid), 128))


def decode_hdr(data: bytes) -> np.ndarray:
    """st_decode_hdr: Radiance .hdr bytes -> (H, W, 3) float32, row 0 the top of the image."""
    lib = load_library()
    fn = lib.st_decode_hdr
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    w, h = C.c_uint32(), C.c_uint32()
    data = bytes(data)
    status = fn(data, len(data), None, 0, C.byref(w), C.byref(h))
    if status == 0:
        out = np.empty((h.value, w.value, 3), np.float32)
        status = fn(data, len(data), out.ctypes.data, out.size, C.byref(w), C.byref(h))
    if status != 0:
        lib.st_last_error.restype = C.c_char_p
        raise StrolleError(f"{_STATUS.get(status, 'error')} (status {status}): {lib.st_last_error().decode(errors='replace')}")
    return out


def decode_cube(data: bytes) -> np.ndarray:
    """st_decode_cube: the text of a .cube file -> (N, N, N, 3) float32 indexed [b, g, r], ready for Engine.insert_lut."""
    lib = load_library()
    fn = lib.st_decode_cube
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    n = C.c_uint32()
    data = bytes(data)
    status = fn(data, len(data), None, 0, C.byref(n))
    if status == 0:
        out = np.empty((n.value, n.value, n.value, 3), np.float32)
        status = fn(data, len(data), out.ctypes.data, out.size, C.byref(n))
    if status != 0:
        lib.st_last_error.restype = C.c_char_p
        raise StrolleError(f"{_STATUS.get(status, 'error')} (status {status}): {lib.st_last_error().decode(errors='replace')}")
    return out


def load_cube(path) -> np.ndarray:
    """A .cube file -> (N, N, N, 3) float32 (st_decode_cube)."""
    with open(path, "rb") as f:
        return decode_cube(f.read())


def load_hdr(path) -> np.ndarray:
    """A Radiance .hdr file -> (H, W, 3) float32 (st_decode_hdr), ready for Engine.set_environment."""
    with open(path, "rb") as f:
        return decode_hdr(f.read())


def decode_png(data: bytes) -> np.ndarray:
    """st_decode_png: PNG bytes -> [h, w, 4] uint8 (the decoder st_scene_load_gltf uses for textures)."""
    return _decode(data, "st_decode_png")


def decode_image(data: bytes) -> np.ndarray:
    """st_decode_image: PNG or JPEG bytes -> [h, w, 4] uint8."""
    return _decode(data, "st_decode_image")


def _decode(data: bytes, symbol: str) -> np.ndarray:
    lib = load_library()
    fn = getattr(lib, symbol)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    w, h = C.c_uint32(), C.c_uint32()
    data = bytes(data)
    status = fn(data, len(data), None, 0, C.byref(w), C.byref(h))
    if status == 0:
        out = np.empty((h.value, w.value, 4), np.uint8)
        status = fn(data, len(data), out.ctypes.data, out.nbytes, C.byref(w), C.byref(h))
    if status != 0:
        lib.st_last_error.restype = C.c_char_p
        raise StrolleError(f"{_STATUS.get(status, 'error')} (status {status}): {lib.st_last_error().decode(errors='replace')}")
    return out
