"""ctypes binding of libvulkansift.so — the vksift_* C API served by HIP kernels on MI355X.

This module is a thin mirror of include/vulkansift/vulkansift.h (+ vksift_ext.h): same function
names, same argument meaning, same error behaviour (void functions report through the configured
error callback). It exists so that the parity tests and bench.py can drive the C-ABI from Python;
it contains no algorithmic code and never falls back to a CPU implementation — importing it
without the built shared library raises.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# VKSIFT_LIB selects another build of the same library (A/B runs of compiler options); never a different implementation
LIB_PATH = os.environ.get("VKSIFT_LIB") or os.path.join(_PKG, "lib", "libvulkansift.so")

VKSIFT_SUCCESS, VKSIFT_INVALID_INPUT_ERROR, VKSIFT_VULKAN_ERROR = 0, 1, 2
VKSIFT_NO_LOG, VKSIFT_LOG_ERROR, VKSIFT_LOG_WARNING, VKSIFT_LOG_INFO, VKSIFT_LOG_DEBUG = range(5)
VKSIFT_DESCRIPTOR_FORMAT_UBC, VKSIFT_DESCRIPTOR_FORMAT_VLFEAT = 0, 1
VKSIFT_PYRAMID_PRECISION_FLOAT32, VKSIFT_PYRAMID_PRECISION_FLOAT16 = 0, 1

ERROR_CB = C.CFUNCTYPE(None, C.c_int)


class vksift_ExternalWindowInfo(C.Structure):
    _fields_ = [("context", C.c_void_p), ("window", C.c_void_p)]


class vksift_Config(C.Structure):
    _fields_ = [
        ("input_image_max_size", C.c_uint32),
        ("sift_buffer_count", C.c_uint32),
        ("max_nb_sift_per_buffer", C.c_uint32),
        ("use_input_upsampling", C.c_bool),
        ("nb_octaves", C.c_uint8),
        ("nb_scales_per_octave", C.c_uint8),
        ("input_image_blur_level", C.c_float),
        ("seed_scale_sigma", C.c_float),
        ("intensity_threshold", C.c_float),
        ("edge_threshold", C.c_float),
        ("max_nb_orientation_per_keypoint", C.c_uint32),
        ("descriptor_format", C.c_int),
        ("gpu_device_index", C.c_int32),
        ("use_hardware_interpolated_blur", C.c_bool),
        ("pyramid_precision_mode", C.c_int),
        ("on_error_callback_function", ERROR_CB),
        ("use_gpu_debug_functions", C.c_bool),
        ("gpu_debug_external_window_info", vksift_ExternalWindowInfo),
    ]


assert C.sizeof(vksift_Config) == 88, C.sizeof(vksift_Config)


class vksift_ext_DetectTimings(C.Structure):
    _fields_ = [
        ("upload_ms", C.c_float), ("pyramid_ms", C.c_float), ("extrema_ms", C.c_float), ("orientation_ms", C.c_float),
        ("descriptor_ms", C.c_float), ("total_ms", C.c_float), ("nb_blur_launches", C.c_uint32), ("pyramid_algorithmic_bytes", C.c_uint64),
        ("scan_ms", C.c_float), ("scan_algorithmic_bytes", C.c_uint64),
        ("pyramid_all_ms", C.c_float), ("nb_blur_launches_all", C.c_uint32),
    ]


FEATURE_DTYPE = np.dtype(
    [
        ("x", "<f4"), ("y", "<f4"), ("scale_x", "<f4"), ("scale_y", "<f4"),
        ("scale_idx", "<u4"), ("octave_idx", "<i4"),
        ("sigma", "<f4"), ("orientation", "<f4"), ("intensity", "<f4"),
        ("descriptor", "u1", (128,)),
    ]
)
MATCH_DTYPE = np.dtype([("idx_a", "<u4"), ("idx_b1", "<u4"), ("idx_b2", "<u4"), ("dist_a_b1", "<f4"), ("dist_a_b2", "<f4")])
FILTERED_MATCH_DTYPE = np.dtype([("idx_a", "<u4"), ("idx_b", "<u4"), ("dist_a_b1", "<f4"), ("dist_a_b2", "<f4")])
HOMOGRAPHY_DTYPE = np.dtype([("H", "<f4", (3, 3)), ("nb_matches", "<u4"), ("nb_inliers", "<u4"), ("best_hypothesis", "<u4"), ("valid", "<u4")])
FUNDAMENTAL_DTYPE = np.dtype([("F", "<f4", (3, 3)), ("nb_matches", "<u4"), ("nb_inliers", "<u4"), ("best_hypothesis", "<u4"), ("best_root", "<u4"), ("valid", "<u4")])
REFINED_HOMOGRAPHY_DTYPE = np.dtype([("H", "<f4", (3, 3)), ("nb_matches", "<u4"), ("nb_inliers", "<u4"), ("rounds", "<u4"), ("valid", "<u4")])
REFINED_FUNDAMENTAL_DTYPE = np.dtype([("F", "<f4", (3, 3)), ("nb_matches", "<u4"), ("nb_inliers", "<u4"), ("rounds", "<u4"), ("valid", "<u4")])
# a caller-supplied keypoint (vksift_ext_Keypoint): image pixels; `response` travels into the feature's intensity field
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("sigma", "<f4"), ("orientation", "<f4"), ("response", "<f4")])
DESCRIBE_ORIENT, DESCRIBE_GIVEN = 0, 1
assert KEYPOINT_DTYPE.itemsize == 20
assert FUNDAMENTAL_DTYPE.itemsize == 56 and REFINED_HOMOGRAPHY_DTYPE.itemsize == 52 and REFINED_FUNDAMENTAL_DTYPE.itemsize == 52
assert FEATURE_DTYPE.itemsize == 164 and MATCH_DTYPE.itemsize == 20 and FILTERED_MATCH_DTYPE.itemsize == 16 and HOMOGRAPHY_DTYPE.itemsize == 52

_lib = None


def lib():
    """Load libvulkansift.so (raises if it has not been built: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -m vulkansift_amd.build` (hipcc, gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    inst, u32, u8 = C.c_void_p, C.c_uint32, C.c_uint8
    L.vksift_loadVulkan.restype = C.c_int
    L.vksift_unloadVulkan.restype = None
    L.vksift_getAvailableGPUs.argtypes = [C.POINTER(u32), C.c_void_p]
    L.vksift_setLogLevel.argtypes = [C.c_int]
    L.vksift_createInstance.argtypes = [C.POINTER(inst), C.POINTER(vksift_Config)]
    L.vksift_createInstance.restype = C.c_int
    L.vksift_destroyInstance.argtypes = [C.POINTER(inst)]
    L.vksift_getDefaultConfig.restype = vksift_Config
    L.vksift_detectFeatures.argtypes = [inst, C.c_void_p, u32, u32, u32]
    L.vksift_matchFeatures.argtypes = [inst, u32, u32]
    L.vksift_getFeaturesNumber.argtypes = [inst, u32]
    L.vksift_getFeaturesNumber.restype = u32
    L.vksift_downloadFeatures.argtypes = [inst, C.c_void_p, u32]
    L.vksift_uploadFeatures.argtypes = [inst, C.c_void_p, u32, u32]
    L.vksift_getMatchesNumber.argtypes = [inst]
    L.vksift_getMatchesNumber.restype = u32
    L.vksift_downloadMatches.argtypes = [inst, C.c_void_p]
    L.vksift_isBufferAvailable.argtypes = [inst, u32]
    L.vksift_isBufferAvailable.restype = C.c_bool
    L.vksift_getScaleSpaceNbOctaves.argtypes = [inst]
    L.vksift_getScaleSpaceNbOctaves.restype = u8
    L.vksift_getScaleSpaceOctaveResolution.argtypes = [inst, u8, C.POINTER(u32), C.POINTER(u32)]
    L.vksift_downloadScaleSpaceImage.argtypes = [inst, u8, u8, C.c_void_p]
    L.vksift_downloadDoGImage.argtypes = [inst, u8, u8, C.c_void_p]
    L.vksift_presentDebugFrame.argtypes = [inst]
    # extensions
    L.vksift_ext_createInstanceBatched.argtypes = [C.POINTER(inst), C.POINTER(vksift_Config), u32]
    L.vksift_ext_createInstanceBatched.restype = C.c_int
    L.vksift_ext_detectFeaturesBatch.argtypes = [inst, C.POINTER(C.c_void_p), u32, u32, u32, u32]
    L.vksift_ext_detectFeaturesBatchDevice.argtypes = [inst, C.c_void_p, u32, u32, u32, u32]
    L.vksift_ext_matchFeaturesBatch.argtypes = [inst, u32, C.POINTER(u32), C.POINTER(u32)]
    L.vksift_ext_getMatchesNumberBatch.argtypes = [inst, u32]
    L.vksift_ext_getMatchesNumberBatch.restype = u32
    L.vksift_ext_downloadMatchesBatch.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_matchFeaturesFiltered.argtypes = [inst, u32, C.POINTER(u32), C.POINTER(u32), C.c_float, C.c_bool]
    L.vksift_ext_getFilteredMatchesNumber.argtypes = [inst, u32]
    L.vksift_ext_getFilteredMatchesNumber.restype = u32
    L.vksift_ext_downloadFilteredMatches.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_verifyHomography.argtypes = [inst, u32, C.c_float, C.c_uint64]
    L.vksift_ext_verifyHomography.restype = None
    L.vksift_ext_getHomography.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_getHomography.restype = None
    L.vksift_ext_downloadInlierMask.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_downloadInlierMask.restype = None
    L.vksift_ext_verifyFundamental.argtypes = [inst, u32, C.c_float, C.c_uint64]
    L.vksift_ext_verifyFundamental.restype = None
    L.vksift_ext_getFundamental.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_getFundamental.restype = None
    L.vksift_ext_downloadFundamentalInlierMask.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_downloadFundamentalInlierMask.restype = None
    L.vksift_ext_getVerifyTime.argtypes = [inst]
    L.vksift_ext_getVerifyTime.restype = C.c_float
    L.vksift_ext_refineHomography.argtypes = [inst, u32, C.c_float]
    L.vksift_ext_refineHomography.restype = None
    L.vksift_ext_getRefinedHomography.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_getRefinedHomography.restype = None
    L.vksift_ext_downloadRefinedInlierMask.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_downloadRefinedInlierMask.restype = None
    L.vksift_ext_getRefineTime.argtypes = [inst]
    L.vksift_ext_getRefineTime.restype = C.c_float
    L.vksift_ext_refineFundamental.argtypes = [inst, u32, C.c_float]
    L.vksift_ext_refineFundamental.restype = None
    L.vksift_ext_getRefinedFundamental.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_getRefinedFundamental.restype = None
    L.vksift_ext_downloadRefinedFundamentalInlierMask.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_downloadRefinedFundamentalInlierMask.restype = None
    L.vksift_ext_getRefineFundamentalTime.argtypes = [inst]
    L.vksift_ext_getRefineFundamentalTime.restype = C.c_float
    L.vksift_ext_matchFeaturesGuided.argtypes = [inst, u32, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_bool]
    L.vksift_ext_matchFeaturesGuided.restype = None
    L.vksift_ext_getGuidedMatchesNumber.argtypes = [inst, u32]
    L.vksift_ext_getGuidedMatchesNumber.restype = u32
    L.vksift_ext_downloadGuidedMatches.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_downloadGuidedMatches.restype = None
    L.vksift_ext_getGuidedMatchTime.argtypes = [inst]
    L.vksift_ext_getGuidedMatchTime.restype = C.c_float
    L.vksift_ext_buildTracks.argtypes = [inst, u32]
    L.vksift_ext_buildTracks.restype = None
    L.vksift_ext_getTrackStats.argtypes = [inst, C.c_void_p]
    L.vksift_ext_getTrackStats.restype = None
    L.vksift_ext_downloadTracks.argtypes = [inst, C.c_void_p]
    L.vksift_ext_downloadTracks.restype = None
    L.vksift_ext_downloadFeatureTracks.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_downloadFeatureTracks.restype = None
    L.vksift_ext_getTracksTime.argtypes = [inst]
    L.vksift_ext_getTracksTime.restype = C.c_float
    L.vksift_ext_beginTrackAccumulation.argtypes = [inst, u32]
    L.vksift_ext_beginTrackAccumulation.restype = None
    L.vksift_ext_accumulateTrackEdges.argtypes = [inst, u32]
    L.vksift_ext_accumulateTrackEdges.restype = None
    L.vksift_ext_getTrackEdgeStats.argtypes = [inst, C.c_void_p]
    L.vksift_ext_getTrackEdgeStats.restype = None
    L.vksift_ext_downloadTrackEdges.argtypes = [inst, C.c_void_p]
    L.vksift_ext_downloadTrackEdges.restype = None
    L.vksift_ext_buildTracksAccumulated.argtypes = [inst]
    L.vksift_ext_buildTracksAccumulated.restype = None
    L.vksift_ext_getAccumulateTime.argtypes = [inst]
    L.vksift_ext_getAccumulateTime.restype = C.c_float
    L.vksift_ext_selectTrackObservations.argtypes = [inst, u32, u32, u32]
    L.vksift_ext_selectTrackObservations.restype = None
    for name in ("getObservationStats", "downloadObservationOffsets", "downloadObservationTrackIds", "downloadObservations"):
        getattr(L, "vksift_ext_" + name).argtypes = [inst, C.c_void_p]
        getattr(L, "vksift_ext_" + name).restype = None
    L.vksift_ext_getObservationsTime.argtypes = [inst]
    L.vksift_ext_getObservationsTime.restype = C.c_float
    L.vksift_ext_triangulateTracks.argtypes = [inst, C.c_void_p, C.c_float, C.c_float]
    L.vksift_ext_triangulateTracks.restype = None
    for name in ("getPointStats", "downloadPoints"):
        getattr(L, "vksift_ext_" + name).argtypes = [inst, C.c_void_p]
        getattr(L, "vksift_ext_" + name).restype = None
    L.vksift_ext_getTriangulateTime.argtypes = [inst]
    L.vksift_ext_getTriangulateTime.restype = C.c_float
    L.vksift_ext_indexObservationsByView.argtypes = [inst]
    L.vksift_ext_indexObservationsByView.restype = None
    L.vksift_ext_refineCameras.argtypes = [inst, u32]
    L.vksift_ext_refineCameras.restype = None
    for name in ("getViewStats", "downloadViewOffsets", "downloadViewObservations", "getCameraStats", "downloadRefinedCameras"):
        getattr(L, "vksift_ext_" + name).argtypes = [inst, C.c_void_p]
        getattr(L, "vksift_ext_" + name).restype = None
    for name in ("getIndexViewsTime", "getRefineCamerasTime"):
        getattr(L, "vksift_ext_" + name).argtypes = [inst]
        getattr(L, "vksift_ext_" + name).restype = C.c_float
    L.vksift_ext_keepStrongestFeatures.argtypes = [inst, u32, u32, u32]
    L.vksift_ext_keepStrongestFeatures.restype = None
    L.vksift_ext_getKeepStrongestTime.argtypes = [inst]
    L.vksift_ext_getKeepStrongestTime.restype = C.c_float
    L.vksift_ext_keepStrongestFeaturesGrid.argtypes = [inst, u32, u32, u32, u32, u32, u32, u32]
    L.vksift_ext_keepStrongestFeaturesGrid.restype = None
    L.vksift_ext_getKeepStrongestGridTime.argtypes = [inst]
    L.vksift_ext_getKeepStrongestGridTime.restype = C.c_float
    L.vksift_ext_convertToRootSift.argtypes = [inst, u32, u32]
    L.vksift_ext_convertToRootSift.restype = None
    L.vksift_ext_getRootSiftTime.argtypes = [inst]
    L.vksift_ext_getRootSiftTime.restype = C.c_float
    L.vksift_ext_describeKeypoints.argtypes = [inst, C.c_void_p, u32, u32, C.c_void_p, u32, u32, u32]
    L.vksift_ext_describeKeypoints.restype = None
    L.vksift_ext_describeKeypointsBatch.argtypes = [inst, C.POINTER(C.c_void_p), u32, u32, u32, C.c_void_p, C.POINTER(u32), u32, u32]
    L.vksift_ext_describeKeypointsBatch.restype = None
    L.vksift_ext_getPlacedKeypointsNumber.argtypes = [inst, u32]
    L.vksift_ext_getPlacedKeypointsNumber.restype = u32
    L.vksift_ext_setProfiling.argtypes = [inst, C.c_bool]
    L.vksift_ext_getDetectTimings.argtypes = [inst, C.POINTER(vksift_ext_DetectTimings)]
    L.vksift_ext_getAccumulatedDetectTimings.argtypes = [inst, C.POINTER(vksift_ext_DetectTimings), C.POINTER(u32), C.c_bool]
    L.vksift_ext_getDetectTimingsSized.argtypes = [inst, C.POINTER(vksift_ext_DetectTimings), C.c_size_t]
    L.vksift_ext_pinHostMemory.argtypes = [C.c_void_p, C.c_size_t]
    L.vksift_ext_pinHostMemory.restype = C.c_int
    L.vksift_ext_unpinHostMemory.argtypes = [C.c_void_p]
    L.vksift_ext_unpinHostMemory.restype = C.c_int
    L.vksift_ext_getScaleSpacePlacement.argtypes = [inst, C.POINTER(C.c_float), C.POINTER(u32)]
    L.vksift_ext_getScaleSpacePlacement.restype = u32
    L.vksift_ext_getAccumulatedDetectTimingsSized.argtypes = [inst, C.POINTER(vksift_ext_DetectTimings), C.c_size_t, C.POINTER(u32), C.c_bool]
    L.vksift_ext_getDeferredStats.argtypes = [inst, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.vksift_ext_getDeferredStats.restype = None
    L.vksift_ext_getMatchTime.argtypes = [inst]
    L.vksift_ext_getMatchTime.restype = C.c_float
    L.vksift_ext_exportDescriptorsDevice.argtypes = [inst, u32, C.c_void_p]
    L.vksift_ext_exportDescriptorsDevice.restype = u32
    L.vksift_ext_genSyntheticImage.argtypes = [C.c_uint64, u32, u32, u32, C.c_void_p]
    L.vksift_ext_genSyntheticDescriptors.argtypes = [C.c_uint64, u32, C.c_void_p]
    L.vksift_ext_genSyntheticImageFamily.argtypes = [C.c_uint64, u32, u32, u32, C.c_void_p]
    L.vksift_ext_genSyntheticImageFamily.restype = None
    L.vksift_ext_shardGetUniqueId.argtypes = [C.c_void_p]
    L.vksift_ext_shardGetUniqueId.restype = C.c_int
    L.vksift_ext_shardGroupCreate.argtypes = [C.POINTER(C.c_void_p), C.c_int, u32, u32, C.c_void_p]
    L.vksift_ext_shardGroupCreate.restype = C.c_int
    L.vksift_ext_shardGroupDestroy.argtypes = [C.POINTER(C.c_void_p)]
    L.vksift_ext_matchSharded.argtypes = [C.c_void_p, C.c_void_p, u32, u32, C.c_void_p, u32, u32, C.c_void_p]
    L.vksift_ext_matchSharded.restype = C.c_int
    L.vksift_ext_shardGroupReserve.argtypes = [C.c_void_p, u32, u32]
    L.vksift_ext_shardGroupReserve.restype = C.c_int
    L.vksift_ext_shardGroupSynchronize.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.vksift_ext_shardGroupSynchronize.restype = C.c_int
    L.vksift_ext_shardGroupCreateWithTransport.argtypes = [C.POINTER(C.c_void_p), C.c_int, u32, u32, C.c_void_p, C.c_void_p]
    L.vksift_ext_shardGroupCreateWithTransport.restype = C.c_int
    L.vksift_ext_shardGroupInfo.argtypes = [C.c_void_p, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.vksift_ext_shardGroupInfo.restype = None
    L.vksift_ext_shardGroupLayout.argtypes = [u32, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.vksift_ext_shardGroupLayout.restype = None
    # kernel-layer C-ABI (include/vksift_hip.h) entry points used directly by bench.py / tests
    for name in ("vksift_hip_memcpy_h2d", "vksift_hip_memcpy_d2h", "vksift_hip_memcpy_d2d"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        getattr(L, name).restype = C.c_int
    L.vksift_hip_stream_sync.argtypes = [C.c_void_p]
    L.vksift_hip_stream_sync.restype = C.c_int
    L.vksift_hip_match_2nn_desc.argtypes = [C.c_void_p, u32, u32, C.c_void_p, u32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.vksift_hip_match_scratch_u32.argtypes = [u32, u32]
    L.vksift_hip_match_scratch_u32.restype = C.c_size_t
    L.vksift_hip_abi_version.argtypes = []
    L.vksift_hip_abi_version.restype = u32
    L.vksift_hip_match_2nn_desc.restype = C.c_int
    L.vksift_hip_gather_descriptors.argtypes = [C.c_void_p, u32, C.c_void_p, C.c_void_p]
    L.vksift_hip_gather_descriptors.restype = C.c_int
    L.vksift_hip_ransac_scratch_u32.argtypes = [u32, u32]
    L.vksift_hip_ransac_scratch_u32.restype = C.c_size_t
    L.vksift_hip_ransac_homography.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, u32, u32, u32, u32, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p,
                                               C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p]
    L.vksift_hip_ransac_homography.restype = C.c_int
    L.vksift_hip_ransac_fundamental.argtypes = L.vksift_hip_ransac_homography.argtypes
    L.vksift_hip_ransac_fundamental.restype = C.c_int
    L.vksift_hip_refit_homography.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, u32, u32, u32, C.c_void_p, C.c_void_p, C.c_uint64, u32, C.c_float, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
    L.vksift_hip_refit_homography.restype = C.c_int
    L.vksift_hip_refit_fundamental.argtypes = L.vksift_hip_refit_homography.argtypes
    L.vksift_hip_refit_fundamental.restype = C.c_int
    L.vksift_hip_guided_scratch_u32.argtypes = [u32, u32]
    L.vksift_hip_guided_scratch_u32.restype = C.c_size_t
    L.vksift_hip_match_guided.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, u32, C.c_void_p, C.c_uint64, C.c_void_p, u32, u32,
                                          C.c_void_p, u32, C.c_void_p, u32, u32, C.c_float, C.c_float, C.c_float, u32, u32, C.c_void_p, C.c_uint64, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p]
    L.vksift_hip_match_guided.restype = C.c_int
    L.vksift_hip_tracks_scratch_u32.argtypes = [u32, u32]
    L.vksift_hip_tracks_scratch_u32.restype = C.c_size_t
    L.vksift_hip_build_tracks.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, u32, u32, C.c_void_p, C.c_uint64, C.c_void_p, u32, C.c_void_p, u32, u32, C.c_void_p, u32,
                                          C.c_void_p, u32, u32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.vksift_hip_build_tracks.restype = C.c_int
    L.vksift_hip_track_edges_scratch_u32.argtypes = [u32, u32]
    L.vksift_hip_track_edges_scratch_u32.restype = C.c_size_t
    L.vksift_hip_append_track_edges.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, u32, u32, C.c_void_p, C.c_uint64, C.c_void_p, u32, C.c_void_p, u32, u32, C.c_void_p, u32,
                                                C.c_void_p, u32, C.c_void_p, u32, C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.vksift_hip_append_track_edges.restype = C.c_int
    L.vksift_hip_build_tracks_from_edges.argtypes = [C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, C.c_void_p, u32, C.c_void_p, u32, u32, C.c_void_p, C.c_void_p, C.c_uint64,
                                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.vksift_hip_build_tracks_from_edges.restype = C.c_int
    L.vksift_hip_observations_scratch_u32.argtypes = [u32, u32, u32]
    L.vksift_hip_observations_scratch_u32.restype = C.c_size_t
    L.vksift_hip_track_observations.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, u32, C.c_void_p, C.c_uint64, C.c_void_p, u32,
                                                C.c_void_p, C.c_void_p, u32, u32, u32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                                C.c_void_p, C.c_size_t, C.c_void_p]
    L.vksift_hip_track_observations.restype = C.c_int
    L.vksift_hip_triangulate_tracks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_float, C.c_float, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.vksift_hip_triangulate_tracks.restype = C.c_int
    L.vksift_hip_views_scratch_u32.argtypes = [C.c_uint64]
    L.vksift_hip_views_scratch_u32.restype = C.c_size_t
    L.vksift_hip_index_views.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.vksift_hip_index_views.restype = C.c_int
    L.vksift_hip_refine_cameras.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, u32, C.c_void_p, u32, u32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vksift_hip_refine_cameras.restype = C.c_int
    _lib = L
    return L


class VksiftError(RuntimeError):
    def __init__(self, code):
        super().__init__({1: "VKSIFT_INVALID_INPUT_ERROR", 2: "VKSIFT_VULKAN_ERROR"}.get(code, str(code)))
        self.code = code


_pending_error = []


@ERROR_CB
def _raising_callback(code):
    # ctypes cannot unwind a Python exception through C frames; record and re-raise on return.
    _pending_error.append(code)


def _check_pending():
    if _pending_error:
        code = _pending_error.pop()
        _pending_error.clear()
        raise VksiftError(code)


_loaded = False


def load():
    global _loaded
    if not _loaded:
        r = lib().vksift_loadVulkan()
        if r != VKSIFT_SUCCESS:
            raise VksiftError(r)
        _loaded = True


def unload():
    global _loaded
    if _loaded:
        lib().vksift_unloadVulkan()
        _loaded = False


def default_config(**overrides):
    cfg = lib().vksift_getDefaultConfig()
    cfg.on_error_callback_function = _raising_callback
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def available_gpus():
    n = C.c_uint32(0)
    lib().vksift_getAvailableGPUs(C.byref(n), None)
    names = (C.c_char * 256 * max(n.value, 1))()
    lib().vksift_getAvailableGPUs(C.byref(n), names)
    return [names[i].value.decode() for i in range(n.value)]


def gen_synthetic_image(seed, width, height, nb_blobs=0):
    out = np.empty((height, width), np.uint8)
    lib().vksift_ext_genSyntheticImage(seed, width, height, nb_blobs, out.ctypes.data)
    return out


SYNTH_BLOBS, SYNTH_EDGES, SYNTH_FRACTAL = 0, 1, 2


def gen_synthetic_image_family(seed, width, height, family):
    """vksift_ext_genSyntheticImageFamily: SYNTH_EDGES (step edges, corners, checker patches) or SYNTH_FRACTAL (1/f noise)"""
    out = np.empty((height, width), np.uint8)
    lib().vksift_ext_genSyntheticImageFamily(seed, width, height, family, out.ctypes.data)
    return out


def gen_synthetic_descriptors(seed, rows):
    out = np.empty((rows, 128), np.uint8)
    lib().vksift_ext_genSyntheticDescriptors(seed, rows, out.ctypes.data)
    return out


def _ransac(entry, words_per_result, dtype, corr, n, nb_hypotheses, threshold_px, seed, scratch_u32):
    import torch

    assert corr.is_cuda and corr.dtype == torch.float32 and corr.is_contiguous() and corr.dim() == 3 and corr.shape[2] == 4
    assert n.is_cuda and n.dtype == torch.int32 and n.is_contiguous() and n.numel() == corr.shape[0]
    nslots, max_n = int(corr.shape[0]), int(corr.shape[1])
    need = int(lib().vksift_hip_ransac_scratch_u32(nslots, nb_hypotheses))
    words = need if scratch_u32 is None else scratch_u32
    # poisoned: the scratch needs no initialisation, the outputs are written for every slot
    scratch = torch.full((max(words, 1),), -1, dtype=torch.int32, device=corr.device)
    results = torch.full((nslots, words_per_result), -1, dtype=torch.int32, device=corr.device)
    masks = torch.full((nslots, max(max_n, 1)), 0x55, dtype=torch.uint8, device=corr.device)
    stream = torch.cuda.current_stream().cuda_stream
    err = entry(corr.data_ptr(), max_n * 16, n.data_ptr(), 1, max_n, nslots, nb_hypotheses, threshold_px, seed, results.data_ptr(), masks.data_ptr(),
                max(max_n, 1), scratch.data_ptr(), words, stream)
    torch.cuda.synchronize()
    if err:
        return err, None, None
    return 0, results.cpu().numpy().view(np.uint8).reshape(nslots, 4 * words_per_result).copy().view(dtype).reshape(nslots), masks.cpu().numpy()


def ransac_homography(corr, n, nb_hypotheses, threshold_px, seed, scratch_u32=None):
    """vksift_hip_ransac_homography on torch tensors: corr float32 [nslots, max_n, 4] and n int32 [nslots] on the GPU. Returns (error code,
    results as a HOMOGRAPHY_DTYPE array, masks uint8 [nslots, max_n]); on an error nothing was launched and the other two are None.
    scratch_u32: words of scratch to hand over instead of what vksift_hip_ransac_scratch_u32 asks for (the refusal tests)."""
    return _ransac(lib().vksift_hip_ransac_homography, 13, HOMOGRAPHY_DTYPE, corr, n, nb_hypotheses, threshold_px, seed, scratch_u32)


def ransac_fundamental(corr, n, nb_hypotheses, threshold_px, seed, scratch_u32=None):
    """vksift_hip_ransac_fundamental, as ransac_homography; the results are a FUNDAMENTAL_DTYPE array"""
    return _ransac(lib().vksift_hip_ransac_fundamental, 14, FUNDAMENTAL_DTYPE, corr, n, nb_hypotheses, threshold_px, seed, scratch_u32)


def _refit(entry, start_words, dtype, d_corr, d_n, start_results, start_masks, nb_rounds, threshold_px, overrides, buffers):
    import torch

    assert d_corr.is_cuda and d_corr.dtype == torch.float32 and d_corr.is_contiguous() and d_corr.dim() == 3 and d_corr.shape[2] == 4
    nslots, max_n = int(d_corr.shape[0]), int(d_corr.shape[1])
    rows = max(max_n, 1)
    assert d_n.is_cuda and d_n.dtype == torch.int32 and d_n.is_contiguous() and d_n.numel() == nslots
    assert start_results.is_cuda and start_results.dtype == torch.int32 and start_results.is_contiguous() and start_results.shape == (nslots, start_words)
    assert start_masks.is_cuda and start_masks.dtype == torch.uint8 and start_masks.is_contiguous() and start_masks.shape == (nslots, rows)
    results = torch.full((nslots, 13), -1, dtype=torch.int32, device=d_corr.device)
    masks = torch.full((nslots, rows), 0x55, dtype=torch.uint8, device=d_corr.device)
    if buffers is not None:
        buffers.update(results=results, masks=masks)
    a = {"corr": d_corr.data_ptr(), "corr_stride": max_n * 16, "mask_stride": rows, "nslots": nslots, "masks_out": masks.data_ptr(), "max_n": max_n}
    a.update(overrides or {})
    err = entry(a["corr"], a["corr_stride"], d_n.data_ptr(), 1, a["max_n"], a["nslots"], start_results.data_ptr(), start_masks.data_ptr(),
                a["mask_stride"], nb_rounds, threshold_px, results.data_ptr(), a["masks_out"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if err:
        return err, None, None
    return 0, results.cpu().numpy().view(np.uint8).reshape(nslots, 52).copy().view(dtype).reshape(nslots), masks.cpu().numpy()


def refit_homography(d_corr, d_n, start_results, start_masks, nb_rounds, threshold_px, overrides=None, buffers=None):
    """vksift_hip_refit_homography on torch tensors on the GPU: d_corr float32 [nslots, max_n, 4], d_n int32 [nslots], start_results int32 [nslots, 13] (the
    RANSAC records as words), start_masks uint8 [nslots, max_n]. Returns (error code, records as a REFINED_HOMOGRAPHY_DTYPE array, masks uint8 [nslots, max_n]);
    on an error nothing was launched and the other two are None. overrides: arguments to hand over instead {"corr", "corr_stride", "mask_stride", "nslots",
    "masks_out", "max_n"} (pointers as integers, strides in bytes); buffers: a dict that receives the tensors the launch writes ("results", "masks"), poisoned
    beforehand (the refusal tests)."""
    return _refit(lib().vksift_hip_refit_homography, 13, REFINED_HOMOGRAPHY_DTYPE, d_corr, d_n, start_results, start_masks, nb_rounds, threshold_px, overrides, buffers)


def refit_fundamental(d_corr, d_n, start_results, start_masks, nb_rounds, threshold_px, overrides=None, buffers=None):
    """vksift_hip_refit_fundamental, as refit_homography; start_results int32 [nslots, 14], the records are a REFINED_FUNDAMENTAL_DTYPE array"""
    return _refit(lib().vksift_hip_refit_fundamental, 14, REFINED_FUNDAMENTAL_DTYPE, d_corr, d_n, start_results, start_masks, nb_rounds, threshold_px, overrides, buffers)


GUIDE_HOMOGRAPHY, GUIDE_FUNDAMENTAL = 0, 1
TRACKS_FILTERED, TRACKS_VERIFIED_H, TRACKS_VERIFIED_F, TRACKS_REFINED_H, TRACKS_REFINED_F, TRACKS_GUIDED = range(6)
NO_TRACK = 0xFFFFFFFF
TRACK_DTYPE = np.dtype([("gpu_buffer_id", "<u4"), ("row", "<u4"), ("length", "<u4"), ("nb_buffers", "<u4")])
TRACK_STATS_DTYPE = np.dtype([("nb_tracks", "<u4"), ("nb_conflicting", "<u4"), ("nb_features", "<u4"), ("nb_edges", "<u4")])
TRACK_EDGE_DTYPE = np.dtype([("gpu_buffer_id_a", "<u4"), ("row_a", "<u4"), ("gpu_buffer_id_b", "<u4"), ("row_b", "<u4")])
TRACK_EDGE_STATS_DTYPE = np.dtype([("nb_edges", "<u4"), ("nb_dropped", "<u4"), ("nb_calls", "<u4"), ("nb_changed_buffers", "<u4")])
OBS_KEEP_CONFLICTING, OBS_DROP_CONFLICTING = 0, 1
OBSERVATION_DTYPE = np.dtype([("gpu_buffer_id", "<u4"), ("row", "<u4"), ("x", "<f4"), ("y", "<f4")])
OBSERVATION_STATS_DTYPE = np.dtype([("nb_tracks", "<u4"), ("nb_observations", "<u4"), ("nb_rejected_length", "<u4"), ("nb_rejected_conflicting", "<u4")])
POINT_DEGENERATE, POINT_TOO_LONG, POINT_BEHIND, POINT_ERROR, POINT_ANGLE = 1, 2, 4, 8, 16
TRIANGULATE_MAX_OBSERVATIONS = 1024
POINT_DTYPE = np.dtype([("X", "<f4", (3,)), ("max_sq_error", "<f4"), ("min_cos", "<f4"), ("status", "<u4"), ("steps", "<u4"), ("nb_observations", "<u4")])
POINT_STATS_DTYPE = np.dtype([("nb_points", "<u4"), ("nb_accepted", "<u4"), ("nb_failed", "<u4"), ("nb_rejected", "<u4")])
VIEW_OBSERVATION_DTYPE = np.dtype([("point", "<u4"), ("row", "<u4"), ("x", "<f4"), ("y", "<f4")])
VIEW_STATS_DTYPE = np.dtype([("nb_views", "<u4"), ("nb_observations", "<u4"), ("largest_view", "<u4"), ("reserved", "<u4")])
CAMERA_ABSENT, CAMERA_TOO_FEW, CAMERA_DEGENERATE, CAMERA_BEHIND = 1, 2, 4, 8
CAMERA_MIN_OBSERVATIONS, CAMERA_MAX_STEPS = 6, 8
REFINED_CAMERA_DTYPE = np.dtype([("P", "<f4", (12,)), ("cost_start", "<f4"), ("cost", "<f4"), ("max_sq_error", "<f4"), ("nb_observations", "<u4"), ("steps", "<u4"),
                                 ("status", "<u4")])
CAMERA_STATS_DTYPE = np.dtype([("nb_views", "<u4"), ("nb_refined", "<u4"), ("nb_unchanged", "<u4"), ("nb_failed", "<u4")])


def guided_match(desc_a, xy_a, desc_b, xy_b, n, models, valid, model_kind, t2, ratio, max_distance, cross_check, scratch_u32=None, strides=None, buffers=None):
    """vksift_hip_match_guided on torch tensors on the GPU: desc_a / desc_b uint8 [nslots, max_n, 128] (dense rows), xy_a / xy_b float32 [nslots, max_n, 2],
    n int32 [nslots, 2] = {N_A, N_B}, models float32 [nslots, 9], valid int32 [nslots]; t2 is the squared threshold in pixels. The shifted norms of the rows are
    formed here the way the matcher's cache holds them. Returns (error code, [FILTERED_MATCH_DTYPE array per slot]); on an error nothing was launched and the
    list is None. scratch_u32: words of scratch to hand over instead of what vksift_hip_guided_scratch_u32 asks for; strides: overrides of the row strides
    {"desc", "norm", "xy", "out"} in their own units; buffers: a dict that receives the tensors the launches write ("out", "out_n", "scratch"), each
    filled with -1 beforehand (the refusal tests)."""
    import torch

    nslots, max_n = int(desc_a.shape[0]), int(desc_a.shape[1])
    for d, xy in ((desc_a, xy_a), (desc_b, xy_b)):
        assert d.is_cuda and d.dtype == torch.uint8 and d.shape == (nslots, max_n, 128) and xy.is_cuda and xy.dtype == torch.float32 and xy.shape == (nslots, max_n, 2)
    assert n.is_cuda and n.dtype == torch.int32 and n.shape == (nslots, 2) and n.is_contiguous()
    assert models.is_cuda and models.dtype == torch.float32 and models.shape == (nslots, 9) and models.is_contiguous()
    assert valid.is_cuda and valid.dtype == torch.int32 and valid.shape == (nslots,) and valid.is_contiguous()
    dev = desc_a.device
    rows = max(max_n, 1)
    # cache entry 2 i holds A of slot i, entry 2 i + 1 its B; the coordinates lie the same way
    desc = torch.zeros((nslots, 2, rows, 128), dtype=torch.uint8, device=dev)
    xy = torch.full((nslots, 2, rows, 2), float("nan"), dtype=torch.float32, device=dev)
    desc[:, 0, :max_n], desc[:, 1, :max_n], xy[:, 0, :max_n], xy[:, 1, :max_n] = desc_a, desc_b, xy_a, xy_b
    norm = ((desc.to(torch.int32) - 128) ** 2).sum(dim=3).to(torch.int32).contiguous()
    tab = torch.arange(2 * nslots, dtype=torch.int32, device=dev)
    need = int(lib().vksift_hip_guided_scratch_u32(nslots, max_n))
    words = need if scratch_u32 is None else scratch_u32
    # poisoned: the scratch needs no initialisation, the counts are written for every slot
    scratch = torch.full((max(words, 2),), -1, dtype=torch.int32, device=dev)
    out = torch.full((nslots, rows, 4), -1, dtype=torch.int32, device=dev)
    out_n = torch.full((nslots,), -1, dtype=torch.int32, device=dev)
    if buffers is not None:
        buffers.update(out=out, out_n=out_n, scratch=scratch)
    st = {"desc": rows * 128, "norm": rows, "xy": rows, "out": rows * 16}
    st.update(strides or {})
    err = lib().vksift_hip_match_guided(desc.data_ptr(), st["desc"], norm.data_ptr(), st["norm"], tab.data_ptr(), 2, xy.data_ptr(), st["xy"], n.data_ptr(), 2, max_n,
                                        models.data_ptr(), 9, valid.data_ptr(), 1, model_kind, t2, ratio, max_distance, 1 if cross_check else 0, nslots,
                                        out.data_ptr(), st["out"], out_n.data_ptr(), scratch.data_ptr(), words, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if err:
        return err, None
    cnt = out_n.cpu().numpy()
    rec = out.cpu().numpy()
    return 0, [rec[i, :cnt[i]].copy().view(FILTERED_MATCH_DTYPE).reshape(-1) for i in range(nslots)]


class Instance:
    """Pythonic handle on a vksift_Instance; method names follow the C API without the prefix."""

    def __init__(self, config=None, batch_capacity=1):
        load()
        self.cfg = config if config is not None else default_config()
        self._h = C.c_void_p(None)
        if batch_capacity > 1:
            r = lib().vksift_ext_createInstanceBatched(C.byref(self._h), C.byref(self.cfg), batch_capacity)
        else:
            r = lib().vksift_createInstance(C.byref(self._h), C.byref(self.cfg))
        if r != VKSIFT_SUCCESS:
            self._h = C.c_void_p(None)
            raise VksiftError(r)
        self.batch_capacity = batch_capacity

    def close(self):
        if self._h:
            lib().vksift_destroyInstance(C.byref(self._h))
            self._h = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- pipelines
    def detectFeatures(self, image, gpu_buffer_id):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        assert image.ndim == 2
        lib().vksift_detectFeatures(self._h, image.ctypes.data, image.shape[1], image.shape[0], gpu_buffer_id)
        _check_pending()

    def detectFeaturesRaw(self, ptr, width, height, gpu_buffer_id):
        lib().vksift_detectFeatures(self._h, ptr, width, height, gpu_buffer_id)
        _check_pending()

    def detectFeaturesBatch(self, images, first_gpu_buffer_id):
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        h, w = imgs[0].shape
        assert all(im.shape == (h, w) for im in imgs)
        ptrs = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        lib().vksift_ext_detectFeaturesBatch(self._h, ptrs, len(imgs), w, h, first_gpu_buffer_id)
        _check_pending()

    @staticmethod
    def imagePointerArray(images):
        """the `const uint8_t *const *images` argument of vksift_ext_detectFeaturesBatch for a list of C-contiguous uint8 arrays
        (which must stay alive): a caller that submits the same frame objects again builds it once"""
        assert all(im.dtype == np.uint8 and im.flags["C_CONTIGUOUS"] for im in images)
        return (C.c_void_p * len(images))(*[im.ctypes.data for im in images])

    def detectFeaturesBatchPtrs(self, ptrs, count, width, height, first_gpu_buffer_id):
        lib().vksift_ext_detectFeaturesBatch(self._h, ptrs, count, width, height, first_gpu_buffer_id)
        _check_pending()

    def detectFeaturesBatchDevice(self, dev_ptr, count, width, height, first_gpu_buffer_id):
        lib().vksift_ext_detectFeaturesBatchDevice(self._h, dev_ptr, count, width, height, first_gpu_buffer_id)
        _check_pending()

    def matchFeatures(self, buf_a, buf_b):
        lib().vksift_matchFeatures(self._h, buf_a, buf_b)
        _check_pending()

    def matchFeaturesBatch(self, bufs_a, bufs_b):
        n = len(bufs_a)
        assert n == len(bufs_b)
        a = (C.c_uint32 * n)(*bufs_a)
        b = (C.c_uint32 * n)(*bufs_b)
        lib().vksift_ext_matchFeaturesBatch(self._h, n, a, b)
        _check_pending()

    def matchFeaturesFiltered(self, bufs_a, bufs_b, ratio=0.75, cross_check=True):
        """2-NN A->B (+ B->A), cross-check and Lowe ratio on the GPU (vksift_ext_matchFeaturesFiltered)."""
        n = len(bufs_a)
        assert n == len(bufs_b)
        a = (C.c_uint32 * n)(*bufs_a)
        b = (C.c_uint32 * n)(*bufs_b)
        lib().vksift_ext_matchFeaturesFiltered(self._h, n, a, b, ratio, cross_check)
        _check_pending()

    def downloadFilteredMatches(self, pair=0):
        n = lib().vksift_ext_getFilteredMatchesNumber(self._h, pair)
        _check_pending()
        out = np.zeros(n, FILTERED_MATCH_DTYPE)
        if n:
            lib().vksift_ext_downloadFilteredMatches(self._h, pair, out.ctypes.data)
            _check_pending()
        return out

    def _pair_record(self, fn, dtype, pair):
        """one of the get* accessors of a pair's result record, as a structured scalar"""
        out = np.zeros(1, dtype)
        fn(self._h, pair, out.ctypes.data)
        _check_pending()
        return out[0]

    def _pair_mask(self, fn, pair):
        """one of the download*InlierMask accessors: a bool per filtered match of the pair"""
        n = lib().vksift_ext_getFilteredMatchesNumber(self._h, pair)
        _check_pending()
        out = np.zeros(n, np.uint8)
        fn(self._h, pair, out.ctypes.data)
        _check_pending()
        return out.astype(bool)

    def verifyHomography(self, nb_hypotheses=1024, threshold_px=2.5, seed=0):
        """RANSAC homography of every pair of the last matchFeaturesFiltered call, on the GPU (vksift_ext_verifyHomography)."""
        lib().vksift_ext_verifyHomography(self._h, nb_hypotheses, threshold_px, seed)
        _check_pending()

    def getHomography(self, pair=0):
        """structured scalar (HOMOGRAPHY_DTYPE): H 3x3 float32 (pixels of A -> B, H[2, 2] == 1), nb_matches, nb_inliers, best_hypothesis, valid"""
        return self._pair_record(lib().vksift_ext_getHomography, HOMOGRAPHY_DTYPE, pair)

    def downloadInlierMask(self, pair=0):
        return self._pair_mask(lib().vksift_ext_downloadInlierMask, pair)

    def verifyFundamental(self, nb_hypotheses=1024, threshold_px=2.5, seed=0):
        """RANSAC fundamental matrix of every pair of the last matchFeaturesFiltered call, on the GPU (vksift_ext_verifyFundamental); its results
        are kept beside the homography's, not in their place."""
        lib().vksift_ext_verifyFundamental(self._h, nb_hypotheses, threshold_px, seed)
        _check_pending()

    def getFundamental(self, pair=0):
        """structured scalar (FUNDAMENTAL_DTYPE): F 3x3 float32 (pixels, (xb, yb, 1) F (xa, ya, 1)^T = 0, largest |entry| in [1, 2)), nb_matches,
        nb_inliers, best_hypothesis, best_root, valid"""
        return self._pair_record(lib().vksift_ext_getFundamental, FUNDAMENTAL_DTYPE, pair)

    def downloadFundamentalInlierMask(self, pair=0):
        return self._pair_mask(lib().vksift_ext_downloadFundamentalInlierMask, pair)

    def getVerifyTime(self):
        return lib().vksift_ext_getVerifyTime(self._h)

    def refineHomography(self, nb_rounds=3, threshold_px=2.5):
        """locally optimised refit of every pair's verified homography on its inliers, on the GPU (vksift_ext_refineHomography); its results are kept
        beside the verification's, not in their place."""
        lib().vksift_ext_refineHomography(self._h, nb_rounds, threshold_px)
        _check_pending()

    def getRefinedHomography(self, pair=0):
        """structured scalar (REFINED_HOMOGRAPHY_DTYPE): H 3x3 float32 (pixels of A -> B, H[2, 2] == 1), nb_matches, nb_inliers, rounds, valid"""
        return self._pair_record(lib().vksift_ext_getRefinedHomography, REFINED_HOMOGRAPHY_DTYPE, pair)

    def downloadRefinedInlierMask(self, pair=0):
        return self._pair_mask(lib().vksift_ext_downloadRefinedInlierMask, pair)

    def getRefineTime(self):
        return lib().vksift_ext_getRefineTime(self._h)

    def refineFundamental(self, nb_rounds=3, threshold_px=2.5):
        """locally optimised refit of every pair's verified fundamental matrix on its inliers, on the GPU (vksift_ext_refineFundamental); its results are
        kept beside the verification's and the refined homographies, not in their place."""
        lib().vksift_ext_refineFundamental(self._h, nb_rounds, threshold_px)
        _check_pending()

    def getRefinedFundamental(self, pair=0):
        """structured scalar (REFINED_FUNDAMENTAL_DTYPE): F 3x3 float32 (pixels, largest |entry| in [1, 2)), nb_matches, nb_inliers, rounds, valid"""
        return self._pair_record(lib().vksift_ext_getRefinedFundamental, REFINED_FUNDAMENTAL_DTYPE, pair)

    def downloadRefinedFundamentalInlierMask(self, pair=0):
        return self._pair_mask(lib().vksift_ext_downloadRefinedFundamentalInlierMask, pair)

    def getRefineFundamentalTime(self):
        return lib().vksift_ext_getRefineFundamentalTime(self._h)

    def matchFeaturesGuided(self, model, models=None, threshold_px=2.5, ratio=0.8, max_distance=float("inf"), cross_check=True):
        """guided matching of every pair of the last matchFeaturesFiltered call under its verified model of kind `model` (GUIDE_HOMOGRAPHY /
        GUIDE_FUNDAMENTAL), or under `models` (float32 [pairs, 9] or [pairs, 3, 3]) when given (vksift_ext_matchFeaturesGuided)"""
        ptr = None
        if models is not None:
            models = np.ascontiguousarray(models, dtype=np.float32).reshape(-1, 9)
            ptr = models.ctypes.data
        lib().vksift_ext_matchFeaturesGuided(self._h, model, ptr, threshold_px, ratio, max_distance, cross_check)
        _check_pending()

    def downloadGuidedMatches(self, pair=0):
        n = lib().vksift_ext_getGuidedMatchesNumber(self._h, pair)
        _check_pending()
        out = np.zeros(n, FILTERED_MATCH_DTYPE)
        if n:
            lib().vksift_ext_downloadGuidedMatches(self._h, pair, out.ctypes.data)
            _check_pending()
        return out

    def getGuidedMatchTime(self):
        return lib().vksift_ext_getGuidedMatchTime(self._h)

    def buildTracks(self, source=TRACKS_FILTERED):
        """merges the matches of every pair of the last matchFeaturesFiltered call into feature tracks on the GPU (vksift_ext_buildTracks); `source` is one
        of TRACKS_FILTERED, TRACKS_VERIFIED_H / _F, TRACKS_REFINED_H / _F, TRACKS_GUIDED; asynchronous like the pair stages"""
        lib().vksift_ext_buildTracks(self._h, source)
        _check_pending()

    def getTrackStats(self):
        """{nb_tracks, nb_conflicting, nb_features, nb_edges} of the last buildTracks"""
        out = np.zeros(1, TRACK_STATS_DTYPE)
        lib().vksift_ext_getTrackStats(self._h, out.ctypes.data)
        _check_pending()
        return {k: int(out[0][k]) for k in TRACK_STATS_DTYPE.names}

    def downloadTracks(self):
        """the track records (TRACK_DTYPE), in track order"""
        n = self.getTrackStats()["nb_tracks"]
        out = np.zeros(n, TRACK_DTYPE)
        if n:
            lib().vksift_ext_downloadTracks(self._h, out.ctypes.data)
            _check_pending()
        return out

    def downloadFeatureTracks(self, buffer_id, nb_features=None):
        """uint32 per feature of the buffer, in download order: its track number or NO_TRACK"""
        n = self.getFeaturesNumber(buffer_id) if nb_features is None else nb_features
        out = np.full(n, NO_TRACK, np.uint32)
        lib().vksift_ext_downloadFeatureTracks(self._h, buffer_id, out.ctypes.data)
        _check_pending()
        return out

    def getTracksTime(self):
        return lib().vksift_ext_getTracksTime(self._h)

    def beginTrackAccumulation(self, max_edges):
        """empties the instance's edge store and sets its capacity (vksift_ext_beginTrackAccumulation): the start of tracks across several
        matchFeaturesFiltered calls; waits for what the instance has in flight"""
        lib().vksift_ext_beginTrackAccumulation(self._h, max_edges)
        _check_pending()

    def accumulateTrackEdges(self, source=TRACKS_FILTERED):
        """appends the edges buildTracks(source) would take from the present matching to the edge store (vksift_ext_accumulateTrackEdges); asynchronous
        like the pair stages"""
        lib().vksift_ext_accumulateTrackEdges(self._h, source)
        _check_pending()

    def getTrackEdgeStats(self):
        """{nb_edges, nb_dropped, nb_calls, nb_changed_buffers} of the edge store"""
        out = np.zeros(1, TRACK_EDGE_STATS_DTYPE)
        lib().vksift_ext_getTrackEdgeStats(self._h, out.ctypes.data)
        _check_pending()
        return {k: int(out[0][k]) for k in TRACK_EDGE_STATS_DTYPE.names}

    def downloadTrackEdges(self):
        """the edges the store holds (TRACK_EDGE_DTYPE), in the order they were accumulated"""
        n = self.getTrackEdgeStats()["nb_edges"]
        out = np.zeros(n, TRACK_EDGE_DTYPE)
        if n:
            lib().vksift_ext_downloadTrackEdges(self._h, out.ctypes.data)
            _check_pending()
        return out

    def buildTracksAccumulated(self):
        """the tracks of every edge the store holds, over every buffer its calls named (vksift_ext_buildTracksAccumulated): they replace the instance's
        tracks, and getTrackStats, downloadTracks, downloadFeatureTracks, selectTrackObservations and what follows serve them. downloadFeatureTracks(b)
        then holds the row count of the first call that named b: pass nb_features if the buffer has been rewritten since (getTrackEdgeStats()
        ["nb_changed_buffers"] != 0)"""
        lib().vksift_ext_buildTracksAccumulated(self._h)
        _check_pending()

    def getAccumulateTime(self):
        return lib().vksift_ext_getAccumulateTime(self._h)

    def selectTrackObservations(self, min_length=2, max_length=0, conflicts=OBS_KEEP_CONFLICTING):
        """builds the observation table of the tracks of the last buildTracks on the GPU (vksift_ext_selectTrackObservations): the tracks of at least
        min_length and (unless 0) at most max_length members, without the conflicting ones under OBS_DROP_CONFLICTING; asynchronous like the build"""
        lib().vksift_ext_selectTrackObservations(self._h, min_length, max_length, conflicts)
        _check_pending()

    def getObservationStats(self):
        """{nb_tracks, nb_observations, nb_rejected_length, nb_rejected_conflicting} of the last selectTrackObservations"""
        out = np.zeros(1, OBSERVATION_STATS_DTYPE)
        lib().vksift_ext_getObservationStats(self._h, out.ctypes.data)
        _check_pending()
        return {k: int(out[0][k]) for k in OBSERVATION_STATS_DTYPE.names}

    def downloadObservationOffsets(self):
        """nb_tracks + 1 uint32: the observations of selected track m are offsets[m] .. offsets[m + 1]"""
        out = np.zeros(self.getObservationStats()["nb_tracks"] + 1, np.uint32)
        lib().vksift_ext_downloadObservationOffsets(self._h, out.ctypes.data)
        _check_pending()
        return out

    def downloadObservationTrackIds(self):
        """per selected track its number in downloadTracks()"""
        n = self.getObservationStats()["nb_tracks"]
        out = np.zeros(n, np.uint32)
        if n:
            lib().vksift_ext_downloadObservationTrackIds(self._h, out.ctypes.data)
            _check_pending()
        return out

    def downloadObservations(self):
        """the observation records (OBSERVATION_DTYPE), grouped by selected track"""
        n = self.getObservationStats()["nb_observations"]
        out = np.zeros(n, OBSERVATION_DTYPE)
        if n:
            lib().vksift_ext_downloadObservations(self._h, out.ctypes.data)
            _check_pending()
        return out

    def getObservationsTime(self):
        return lib().vksift_ext_getObservationsTime(self._h)

    def triangulateTracks(self, cameras, threshold_px, cos_min_angle=1.0):
        """triangulates every selected track of the last selectTrackObservations on the GPU (vksift_ext_triangulateTracks). cameras: float32
        [sift_buffer_count, 3, 4] (or None, which the library refuses), row-major P per gpu_buffer_id; a point is accepted when its largest reprojection error
        is below threshold_px and, with cos_min_angle < 1, its largest triangulation angle is wide enough; asynchronous like the selection"""
        if cameras is not None:
            cameras = np.ascontiguousarray(cameras, np.float32)
            assert cameras.size == 12 * self.cfg.sift_buffer_count, "one 3x4 camera per SIFT buffer"
        lib().vksift_ext_triangulateTracks(self._h, None if cameras is None else cameras.ctypes.data, threshold_px, cos_min_angle)
        _check_pending()

    def getPointStats(self):
        """{nb_points, nb_accepted, nb_failed, nb_rejected} of the last triangulateTracks"""
        out = np.zeros(1, POINT_STATS_DTYPE)
        lib().vksift_ext_getPointStats(self._h, out.ctypes.data)
        _check_pending()
        return {k: int(out[0][k]) for k in POINT_STATS_DTYPE.names}

    def downloadPoints(self):
        """the point records (POINT_DTYPE): point m belongs to selected track m of the observation table"""
        n = self.getPointStats()["nb_points"]
        out = np.zeros(n, POINT_DTYPE)
        if n:
            lib().vksift_ext_downloadPoints(self._h, out.ctypes.data)
            _check_pending()
        return out

    def getTriangulateTime(self):
        return lib().vksift_ext_getTriangulateTime(self._h)

    def indexObservationsByView(self):
        """inverts the observation table of the last selectTrackObservations by view on the GPU (vksift_ext_indexObservationsByView); asynchronous like the
        selection"""
        lib().vksift_ext_indexObservationsByView(self._h)
        _check_pending()

    def getViewStats(self):
        """{nb_views, nb_observations, largest_view, reserved} of the last view index"""
        out = np.zeros(1, VIEW_STATS_DTYPE)
        lib().vksift_ext_getViewStats(self._h, out.ctypes.data)
        _check_pending()
        return {k: int(out[0][k]) for k in VIEW_STATS_DTYPE.names}

    def downloadViewOffsets(self):
        """uint32 [sift_buffer_count + 1], indexed by gpu_buffer_id: view b holds the records view_offsets[b] .. view_offsets[b + 1]"""
        out = np.zeros(self.cfg.sift_buffer_count + 1, np.uint32)
        lib().vksift_ext_downloadViewOffsets(self._h, out.ctypes.data)
        _check_pending()
        return out

    def downloadViewObservations(self):
        """the index's records (VIEW_OBSERVATION_DTYPE), grouped by view"""
        n = self.getViewStats()["nb_observations"]
        out = np.zeros(n, VIEW_OBSERVATION_DTYPE)
        if n:
            lib().vksift_ext_downloadViewObservations(self._h, out.ctypes.data)
            _check_pending()
        return out

    def getIndexViewsTime(self):
        return lib().vksift_ext_getIndexViewsTime(self._h)

    def refineCameras(self, nb_steps=4):
        """refines every camera of the last triangulateTracks on the accepted points of its view, the points held fixed, by up to nb_steps Gauss-Newton
        steps on the GPU (vksift_ext_refineCameras); builds the view index first if there is none; asynchronous like the triangulation"""
        lib().vksift_ext_refineCameras(self._h, nb_steps)
        _check_pending()

    def getCameraStats(self):
        """{nb_views, nb_refined, nb_unchanged, nb_failed} of the last refineCameras"""
        out = np.zeros(1, CAMERA_STATS_DTYPE)
        lib().vksift_ext_getCameraStats(self._h, out.ctypes.data)
        _check_pending()
        return {k: int(out[0][k]) for k in CAMERA_STATS_DTYPE.names}

    def downloadRefinedCameras(self):
        """one record per SIFT buffer (REFINED_CAMERA_DTYPE), indexed by gpu_buffer_id; rec["P"].reshape(-1, 3, 4) goes back into triangulateTracks"""
        out = np.zeros(self.cfg.sift_buffer_count, REFINED_CAMERA_DTYPE)
        lib().vksift_ext_downloadRefinedCameras(self._h, out.ctypes.data)
        _check_pending()
        return out

    def getRefineCamerasTime(self):
        return lib().vksift_ext_getRefineCamerasTime(self._h)

    def keepStrongestFeatures(self, first_buffer, count, max_features):
        """every SIFT buffer of [first_buffer, first_buffer + count) keeps its max_features strongest features (|DoG response|, ties by download
        order), selected and compacted on the GPU (vksift_ext_keepStrongestFeatures); asynchronous like detectFeatures"""
        lib().vksift_ext_keepStrongestFeatures(self._h, first_buffer, count, max_features)
        _check_pending()

    def getKeepStrongestTime(self):
        return lib().vksift_ext_getKeepStrongestTime(self._h)

    def keepStrongestFeaturesGrid(self, first_buffer, count, max_features, image_width, image_height, grid_cols, grid_rows):
        """keepStrongestFeatures spread over the image (vksift_ext_keepStrongestFeaturesGrid): every cell of a grid_cols x grid_rows grid over an
        image_width x image_height frame keeps its max_features // cells strongest features first, the strongest of the rest fill the budget up.
        max_features is the total per buffer, not a number per cell; asynchronous like detectFeatures"""
        lib().vksift_ext_keepStrongestFeaturesGrid(self._h, first_buffer, count, max_features, image_width, image_height, grid_cols, grid_rows)
        _check_pending()

    def getKeepStrongestGridTime(self):
        return lib().vksift_ext_getKeepStrongestGridTime(self._h)

    def convertToRootSift(self, first_buffer, count):
        """the descriptors of every SIFT buffer of [first_buffer, first_buffer + count) become RootSIFT descriptors (L1-normalised, square-rooted,
        512 sqrt(d / sum) rounded half up exactly, saturated to 255), in place on the GPU (vksift_ext_convertToRootSift); asynchronous like
        detectFeatures. Not idempotent: a second call converts a second time"""
        lib().vksift_ext_convertToRootSift(self._h, first_buffer, count)
        _check_pending()

    def getRootSiftTime(self):
        return lib().vksift_ext_getRootSiftTime(self._h)

    def describeKeypoints(self, image, keypoints, gpu_buffer_id, mode=DESCRIBE_ORIENT):
        """describe the caller's keypoints (KEYPOINT_DTYPE, image pixels) on `image` into a SIFT buffer (vksift_ext_describeKeypoints): orientations
        from the image (DESCRIBE_ORIENT) or the supplied ones (DESCRIBE_GIVEN); asynchronous like detectFeatures. keypoints None: a NULL list"""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        assert image.ndim == 2
        kps = None if keypoints is None else np.ascontiguousarray(keypoints, dtype=KEYPOINT_DTYPE)
        n = 0 if kps is None else len(kps)
        lib().vksift_ext_describeKeypoints(self._h, image.ctypes.data, image.shape[1], image.shape[0], None if kps is None else kps.ctypes.data, n, gpu_buffer_id, mode)
        _check_pending()

    def describeKeypointsRaw(self, image_ptr, width, height, kps_ptr, nb_kps, gpu_buffer_id, mode):
        lib().vksift_ext_describeKeypoints(self._h, image_ptr, width, height, kps_ptr, nb_kps, gpu_buffer_id, mode)
        _check_pending()

    def describeKeypointsBatch(self, images, keypoint_lists, first_gpu_buffer_id, mode=DESCRIBE_ORIENT):
        """image i with keypoint_lists[i] into SIFT buffer first_gpu_buffer_id + i, one launch sequence (vksift_ext_describeKeypointsBatch)"""
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        h, w = imgs[0].shape
        assert all(im.shape == (h, w) for im in imgs) and len(keypoint_lists) == len(imgs)
        lists = [np.ascontiguousarray(k, dtype=KEYPOINT_DTYPE) for k in keypoint_lists]
        kps = np.concatenate(lists) if lists else np.zeros(0, KEYPOINT_DTYPE)
        ptrs = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        counts = (C.c_uint32 * len(imgs))(*[len(k) for k in lists])
        lib().vksift_ext_describeKeypointsBatch(self._h, ptrs, len(imgs), w, h, kps.ctypes.data if len(kps) else None, counts, first_gpu_buffer_id, mode)
        _check_pending()

    def getPlacedKeypointsNumber(self, gpu_buffer_id):
        """keypoints the buffer's last describe call stored, before orientation copies (vksift_ext_getPlacedKeypointsNumber)"""
        n = lib().vksift_ext_getPlacedKeypointsNumber(self._h, gpu_buffer_id)
        _check_pending()
        return n

    def getMatchesNumberBatch(self, pair):
        n = lib().vksift_ext_getMatchesNumberBatch(self._h, pair)
        _check_pending()
        return n

    def downloadMatchesBatch(self, pair):
        n = self.getMatchesNumberBatch(pair)
        out = np.zeros(n, MATCH_DTYPE)
        if n:
            lib().vksift_ext_downloadMatchesBatch(self._h, pair, out.ctypes.data)
            _check_pending()
        return out

    # -- transfers
    def getFeaturesNumber(self, gpu_buffer_id):
        n = lib().vksift_getFeaturesNumber(self._h, gpu_buffer_id)
        _check_pending()
        return n

    def downloadFeatures(self, gpu_buffer_id):
        n = self.getFeaturesNumber(gpu_buffer_id)
        out = np.zeros(n, FEATURE_DTYPE)
        if n:
            lib().vksift_downloadFeatures(self._h, out.ctypes.data, gpu_buffer_id)
            _check_pending()
        return out

    def uploadFeatures(self, feats, gpu_buffer_id):
        feats = np.ascontiguousarray(feats, dtype=FEATURE_DTYPE)
        lib().vksift_uploadFeatures(self._h, feats.ctypes.data, len(feats), gpu_buffer_id)
        _check_pending()

    def getMatchesNumber(self):
        return lib().vksift_getMatchesNumber(self._h)

    def downloadMatches(self):
        n = self.getMatchesNumber()
        out = np.zeros(n, MATCH_DTYPE)
        lib().vksift_downloadMatches(self._h, out.ctypes.data)
        _check_pending()
        return out

    def isBufferAvailable(self, gpu_buffer_id):
        return bool(lib().vksift_isBufferAvailable(self._h, gpu_buffer_id))

    # -- scale space
    def getScaleSpaceNbOctaves(self):
        return lib().vksift_getScaleSpaceNbOctaves(self._h)

    def getScaleSpaceOctaveResolution(self, octave):
        w, h = C.c_uint32(0), C.c_uint32(0)
        lib().vksift_getScaleSpaceOctaveResolution(self._h, octave, C.byref(w), C.byref(h))
        _check_pending()
        return w.value, h.value

    def downloadScaleSpaceImage(self, octave, scale):
        w, h = self.getScaleSpaceOctaveResolution(octave)
        out = np.zeros((h, w), np.float32)
        lib().vksift_downloadScaleSpaceImage(self._h, octave, scale, out.ctypes.data)
        _check_pending()
        return out

    def downloadDoGImage(self, octave, scale):
        w, h = self.getScaleSpaceOctaveResolution(octave)
        out = np.zeros((h, w), np.float32)
        lib().vksift_downloadDoGImage(self._h, octave, scale, out.ctypes.data)
        _check_pending()
        return out

    def presentDebugFrame(self):
        lib().vksift_presentDebugFrame(self._h)

    # -- extensions
    def setProfiling(self, enabled=True):
        lib().vksift_ext_setProfiling(self._h, enabled)

    def getDetectTimings(self):
        t = vksift_ext_DetectTimings()
        lib().vksift_ext_getDetectTimingsSized(self._h, C.byref(t), C.sizeof(t))
        return {f[0]: getattr(t, f[0]) for f in t._fields_}

    def getAccumulatedDetectTimings(self, reset=False):
        t = vksift_ext_DetectTimings()
        n = C.c_uint32(0)
        lib().vksift_ext_getAccumulatedDetectTimingsSized(self._h, C.byref(t), C.sizeof(t), C.byref(n), reset)
        d = {f[0]: getattr(t, f[0]) for f in t._fields_}
        d["nb_calls"] = n.value
        return d

    def getScaleSpacePlacement(self):
        """candidate memory ranges timed at allocation: {"gbps": [...], "chosen": [...]} (empty lists: plain allocation; one chosen range per scale-space buffer of the instance: one, or two with VKSIFT_PYR_PINGPONG=2)"""
        g = (C.c_float * 8)()
        ch = (C.c_uint32 * 2)()
        n = lib().vksift_ext_getScaleSpacePlacement(self._h, g, ch)
        return {"gbps": [round(float(g[i]), 1) for i in range(n)], "chosen": list(dict.fromkeys([int(ch[0]), int(ch[1])])) if n else []}

    def getMatchTime(self):
        return lib().vksift_ext_getMatchTime(self._h)

    def getDeferredStats(self):
        """(batches launched from staged vksift_detectFeatures calls, images in them) — include/vksift_ext.h"""
        b, n = C.c_uint64(0), C.c_uint64(0)
        lib().vksift_ext_getDeferredStats(self._h, C.byref(b), C.byref(n))
        return int(b.value), int(n.value)

    def exportDescriptorsDevice(self, gpu_buffer_id, dev_ptr):
        n = lib().vksift_ext_exportDescriptorsDevice(self._h, gpu_buffer_id, dev_ptr)
        _check_pending()
        return n
