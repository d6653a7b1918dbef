/*
 * vksift_hip.h — the thin C-ABI between the C host (vulkansift_amd/csrc/host/) and the hand-written
 * HIP kernels for gfx950 (vulkansift_amd/csrc/hip/). Plain pointers, sizes and an opaque stream
 * handle only: no HIP, torch or C++ types appear in any signature, so the same entry points can be
 * bound from C, ctypes or any FFI.
 *
 * Each launch shim replaces one recorded Vulkan command of the reference's detection / matching
 * command buffers (reference file:line given per function; paths relative to src/vulkansift/).
 * All shims are asynchronous on `stream` and return 0 on success or a non-zero hipError_t value.
 *
 * Data layout in HBM:
 *   plane      : fp32, row-major, row pitch `pitch` floats (multiple of 64 floats = 256 B)
 *   octave     : (S+3) Gaussian planes, plane stride = pitch*h floats. DoG planes are not stored: D[s] = G[s+1] - G[s] is
 *                formed in registers where it is consumed (extrema scan, refinement), bit-identically
 *   batch      : image b of a batched detect lives `img_stride` floats after image b-1
 *   SIFT buffer: per octave section of 164-byte vksift_Feature records; counters live in a
 *                separate u32 array (found[o], un-clamped like nb_elem in the reference)
 */
#ifndef VKSIFT_HIP_H
#define VKSIFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C"
{
#endif

#define VKSIFT_HIP_MAX_TAPS 20 /* VKSIFT_DETECTOR_MAX_GAUSSIAN_KERNEL_SIZE, sift_detector.h:9 */
#define VKSIFT_HIP_MATCH_CHUNKS 32   /* partial top-2 lists per A row of the single-pair matcher (merged exactly) */
#define VKSIFT_HIP_MATCH_SMALL_NA 1536u /* single pairs with N_A <= this (and, where the host knows it, N_B <= ..._SMALL_NB) */
#define VKSIFT_HIP_MATCH_SMALL_NB 4096u /* take the one-launch small kernel and need no partial lists */
/* u32 words of scratch vksift_hip_match_2nn_desc needs for na query rows against nb reference rows (norms of A and B, row flags /
 * row list, per-row partial lists of the decomposed kernels: 16 words per piece for the cell scan of large reference sets) */
#define VKSIFT_HIP_MATCH_SCRATCH_U32(na, nb) (2u * (size_t)(na) + (size_t)(nb) + 72u + (size_t)(na) * 16u * VKSIFT_HIP_MATCH_CHUNKS)
#define VKSIFT_HIP_ABI_VERSION 16u     /* bumped whenever a signature or a scratch contract of this header changes (vksift_hip_abi_version); 12: vksift_hip_build_tracks, 13: vksift_hip_track_observations, 14: vksift_hip_triangulate_tracks, 15: vksift_hip_index_views, vksift_hip_refine_cameras, 16: vksift_hip_append_track_edges, vksift_hip_build_tracks_from_edges */
#define VKSIFT_HIP_GATHER_SLOTS 512u   /* SIFT buffers one vksift_hip_gather_sections launch serves */
#define VKSIFT_HIP_MATCH_SLOTS 256u    /* pairs one vksift_hip_match_2nn_async launch sequence serves */
#define VKSIFT_HIP_MATCH_PK_NB 32768u  /* reference sets of at most this many rows take the branch-free packed-key kernel (k_match_pk) */
#define VKSIFT_HIP_MAX_ORI 18  /* a 36-bin circular histogram has at most 18 strict local maxima */
#define VKSIFT_HIP_MAX_OCTAVE_SIDE 16383u /* candidate coordinates are packed 14 + 14 bits: octaves up to 16383 x 16383 texels */

  typedef void *vksift_hip_stream;
  typedef void *vksift_hip_graph; /* an instantiated hipGraph (hipGraphExec_t) */
  typedef void *vksift_hip_event;

  /* ------------------------------------------------------------------ runtime (replaces the vkenv directory) */
  int vksift_hip_init(void);                          /* vulkan_device.c:17 vkenv_createInstance */
  uint32_t vksift_hip_abi_version(void);              /* VKSIFT_HIP_ABI_VERSION the library was built with */
  int vksift_hip_device_count(void);                  /* vulkan_device.c: vkenv_getPhysicalDevicesProperties */
  int vksift_hip_device_name(int idx, char *out256);
  int vksift_hip_set_device(int idx);
  size_t vksift_hip_device_free_mem(void);
  void *vksift_hip_malloc(size_t bytes);              /* NULL on failure */
  void vksift_hip_free(void *p);
  void *vksift_hip_host_malloc(size_t bytes);         /* pinned; replaces HOST_VISIBLE staging buffers */
  void vksift_hip_host_free(void *p);
  int vksift_hip_host_register(void *p, size_t bytes); /* page-lock caller memory: copies into it become DMA transfers */
  int vksift_hip_host_unregister(void *p);
  int vksift_hip_is_pinned(const void *p);             /* 1: page-locked host memory (registered or vksift_hip_host_malloc) */
  vksift_hip_stream vksift_hip_stream_create(void);
  void vksift_hip_stream_destroy(vksift_hip_stream s);
  int vksift_hip_stream_sync(vksift_hip_stream s);    /* vkWaitForFences */
  int vksift_hip_stream_busy(vksift_hip_stream s);    /* vkGetFenceStatus: 1 busy, 0 idle, <0 error */
  vksift_hip_event vksift_hip_event_create(void);
  void vksift_hip_event_destroy(vksift_hip_event e);
  int vksift_hip_event_record(vksift_hip_event e, vksift_hip_stream s);
  int vksift_hip_event_sync(vksift_hip_event e);
  int vksift_hip_event_busy(vksift_hip_event e);
  float vksift_hip_event_elapsed_ms(vksift_hip_event a, vksift_hip_event b);
  int vksift_hip_stream_wait_event(vksift_hip_stream s, vksift_hip_event e);
  /* hipGraph capture of everything enqueued to s (and to streams forked from it through events) between begin and end;
   * the launch-bound single-image pipeline (~100 short kernels) is replayed with one vksift_hip_graph_launch. */
  int vksift_hip_capture_begin(vksift_hip_stream s);
  int vksift_hip_capture_end(vksift_hip_stream s, vksift_hip_graph *out);
  int vksift_hip_graph_launch(vksift_hip_graph g, vksift_hip_stream s);
  void vksift_hip_graph_destroy(vksift_hip_graph g);
  int vksift_hip_memcpy_h2d(void *dst, const void *src, size_t n, vksift_hip_stream s);
  int vksift_hip_memcpy_d2h(void *dst, const void *src, size_t n, vksift_hip_stream s);
  int vksift_hip_memcpy_d2d(void *dst, const void *src, size_t n, vksift_hip_stream s);
  int vksift_hip_memcpy2d_d2h(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t height, vksift_hip_stream s);
  /* kernel store of n_words into a vksift_hip_host_malloc allocation (see runtime.hip: keeps dependent read-backs off the copy engine) */
  int vksift_hip_post_words(uint32_t *host_mapped_dst, const uint32_t *src, size_t n_words, vksift_hip_stream s);
  int vksift_hip_memset(void *dst, int value, size_t n, vksift_hip_stream s);
  const char *vksift_hip_error_string(int err);
  void vksift_hip_range_push(const char *name);       /* roctx marker == VK_EXT_debug_marker region */
  void vksift_hip_range_pop(void);

  /* Development / test knobs of the launch shims (A/B tools, tests of fallback paths). Every setting produces identical results.
   * PROCESS-WIDE and not synchronised: they act on every instance of the process; set them before instances are created (tests, tools),
   * never while another thread is inside a library call. */
  enum
  {
    VKSIFT_TUNE_WG_TARGET = 0,  /* waves per strip-march launch aimed at, for every strip-march launcher (0 = built-in; when set it also
                                 * replaces VKSIFT_TUNE_SEED_WG) */
    VKSIFT_TUNE_WIDE_MASK = 1,  /* bit n: n-tap launches take the four-texels-per-lane form (-1 = built-in) */
    VKSIFT_TUNE_MULTI_MAX = 2,  /* octaves per multi-octave launch, 1..8 (0 = built-in 8): the cutting of longer octave lists into runs is
                                 * otherwise only reached by images of 4097 pixels and more on the shortest side */
    VKSIFT_TUNE_REFINE_PTR = 3, /* 1: the refinement kernels address the scale-space through pointers everywhere (the form octaves beyond
                                 * 2 GiB take) instead of one buffer resource per image and octave */
    VKSIFT_TUNE_SCAN_FORM = 4,  /* development: launch form of the cell-scan matcher (0 = built-in) */
    VKSIFT_TUNE_PAIR_FORM = 5,  /* two-scale blur launch: 0 built-in, 1 two texels per lane, 2 four texels per lane */
    VKSIFT_TUNE_PYR_GATE = 6,   /* 1: the next detection's scale-space starts behind the matching queued before it (default: beside it) */
    VKSIFT_TUNE_DENSE_ROWS = 7, /* 1: the descriptor launch does not write the matcher's dense rows (the gather pass of the first matching does, as
                                 * for uploaded buffers); A/B and the bit-identity matrix */
    VKSIFT_TUNE_SEED_WG = 8,    /* waves aimed at by the fused up-sampling + seed launch (0 = built-in) */
    VKSIFT_TUNE_SCAN_BAND = 9,  /* rows per wave of the streaming extrema scan on octaves of more than 256 rows (0 = built-in: 48 there, and 16 when
                                 * the whole launch has fewer than 2048 waves; octaves of up to 256 rows always take 16) */
    VKSIFT_TUNE_TAIL_MULTI = 10, /* 1: no multi-octave launches for scales S+1, S+2 (batches queue every octave in full; forked detections one launch per
                                  * octave and scale) */
    VKSIFT_TUNE_ZERO_COPY = 11,  /* 1: a single host image is copied into device memory in front of the seed launch (default: the launch reads the pinned
                                  * staging buffer itself) */
    VKSIFT_TUNE_MIN_MARCH = 12,  /* output rows per wave of the smallest strip-march launches (a single image's): 0 = built-in */
    VKSIFT_TUNE_TAIL_FUSED = 13, /* tail of the keypoint extraction (ballots -> records): 0 = built-in (batches of 64 images and more take one launch with one
                                  * workgroup per image and octave, smaller calls the four sparse launches), 1: always the four launches, 2: always the one, 3: as 2 with the 512-thread workgroups that launches
                                  * of 512 workgroups and more take (tests of that form at small sizes) */
    VKSIFT_TUNE_DESC_SOLO_R = 14, /* two-wave descriptor launch (batches of 8 and more): the largest window radius R at which a keypoint is described by one
                                   * wave alone, two such keypoints per workgroup; 0: none (every keypoint on both waves, one keypoint per workgroup), 63 and
                                   * more: every keypoint with R <= 63. Built-in: VKSIFT_HIP_DESC_SOLO_R */
    VKSIFT_TUNE_COUNT = 16
  };
#define VKSIFT_HIP_DESC_SOLO_R 63 /* built-in value of VKSIFT_TUNE_DESC_SOLO_R */
  int vksift_hip_tune(int knob, int value);
  int vksift_hip_tune_get(int knob);

  /* ------------------------------------------------------------------ pyramid */
  /* The launchers below that can decline a shape (vksift_hip_blur_pair, _blur_downsample, _blur_multi, _seed_upsampled, _seed_direct,
   * _octave_chain) return -1 when it is not covered and nothing was launched: the caller then issues the separate calls named in the
   * launcher's comment. 0: launched; a positive value: a hipError_t (invalid arguments or a failed launch). */

  /* A batch of same-sized planes. */
  typedef struct
  {
    float *base;         /* plane of image 0 */
    uint32_t w, h;       /* valid extent */
    uint32_t pitch;      /* floats per row */
    uint64_t img_stride; /* texels between consecutive images of the batch */
    uint32_t fp16;       /* 0: fp32 texels; 1: IEEE binary16 texels (VKSIFT_PYRAMID_PRECISION_FLOAT16: stored round-to-nearest-even,
                          * widened exactly on every read, all arithmetic fp32); base then points at 2-byte texels */
    uint32_t reverse;    /* dispatch-order hint, read from the DESTINATION plane of a launch: 1 = every XCD walks its share of the
                          * (image, row segment, strip) space back to front. Consecutive launches of a chain alternate it, so that
                          * a launch starts on the texels its predecessor touched last — the ones still in the 256 MiB Infinity
                          * Cache — instead of on the ones it evicted first. Results do not depend on it */
  } vksift_hip_Plane;

  /* vkCmdCopyBufferToImage + vkCmdBlitImage(LINEAR) of sift_detector.c:881,909-916:
   * u8 row-major images (src_stride bytes between images) -> fp32 plane, value/255, bilinear 2x (or
   * 1:1 copy when the sizes match), clamp-to-edge. */
  int vksift_hip_input_blit(const uint8_t *src, uint32_t sw, uint32_t sh, uint64_t src_img_stride, vksift_hip_Plane dst, uint32_t batch,
                            vksift_hip_stream s);

  /* One Gaussian scale step = the H and V GaussianBlur*.comp dispatches of sift_detector.c:927-1001
   * fused through LDS. taps[0..ntaps) are one-sided direct weights, centre first; the borders use
   * mirrored-repeat addressing. src and dst must not alias. */
  int vksift_hip_blur(vksift_hip_Plane src, vksift_hip_Plane dst, const float *taps, uint32_t ntaps, uint32_t batch, vksift_hip_stream s);

  /* TWO consecutive scale steps in one launch: dst1 = blur(src, taps1), dst2 = blur(dst1, taps2) — the source plane is read once and
   * scale s never re-read (12 bytes per texel instead of 16). Bit-identical to two vksift_hip_blur calls. -1 when the tap counts, the
   * texel type or the shape are not covered: the caller then issues the two calls. */
  int vksift_hip_blur_pair(vksift_hip_Plane src, vksift_hip_Plane dst1, vksift_hip_Plane dst2, const float *taps1, uint32_t ntaps1, const float *taps2,
                           uint32_t ntaps2, uint32_t batch, vksift_hip_stream s);

  /* the kernel vksift_hip_blur takes for this shape: 0 generic tiles, 1 two texels per lane (what vksift_hip_blur_multi launches), 2 four texels per lane */
  int vksift_hip_blur_form(vksift_hip_Plane src, vksift_hip_Plane dst, uint32_t ntaps, uint32_t batch);

  /* One scale of n <= 8 octaves in ONE launch: dst[i] = blur(src[i]) for every i with the same taps (scales S+1 and S+2 of a detection's octaves
   * feed nothing but the extrema scan, so they can be queued per scale instead of per octave). -1 when a plane is outside the strip-march
   * kernel's domain, the texel types differ or the tap count has no multi-octave instantiation (9, 11, 13, 15 taps exist): the caller then
   * takes vksift_hip_blur per plane. Same kernel body: bit-identical to those launches. */
  int vksift_hip_blur_multi(const vksift_hip_Plane *src, const vksift_hip_Plane *dst, uint32_t n, const float *taps, uint32_t ntaps, uint32_t batch,
                            vksift_hip_stream s);

  /* vksift_hip_blur that also seeds the next octave: next(x, y) = dst(2x+1, 2y+1), the vkCmdBlitImage(NEAREST) of
   * sift_detector.c:1003-1034 for exactly halved sizes, stored from the registers that hold the blurred rows (the separate
   * pass re-reads the whole plane). Bit-identical to vksift_hip_blur + vksift_hip_downsample. -1 when the shape or the selected
   * kernel does not cover it: the caller then issues the two separate calls. */
  int vksift_hip_blur_downsample(vksift_hip_Plane src, vksift_hip_Plane dst, vksift_hip_Plane next, const float *taps, uint32_t ntaps, uint32_t batch,
                                 vksift_hip_stream s);

  /* vkCmdCopyBufferToImage + vkCmdBlitImage(LINEAR, exact 2:1) + the seed blur (sift_detector.c:881-1001 for octave 0) in one
   * pass: dst = blur(upsample2x(src / 255)); the up-sampled plane is never written. Bit-identical to vksift_hip_input_blit
   * followed by vksift_hip_blur. -1 when the shape is not covered: the caller then issues the two separate calls. */
  int vksift_hip_seed_upsampled(const uint8_t *src, uint32_t sw, uint32_t sh, uint64_t src_img_stride, vksift_hip_Plane dst, const float *taps, uint32_t ntaps,
                                uint32_t batch, vksift_hip_stream s);

  /* The same without up-sampling (use_input_upsampling = false: the blit of sift_detector.c:909-916 is a 1:1 copy): dst = blur(src / 255)
   * straight from the u8 images. Bit-identical to vksift_hip_input_blit + vksift_hip_blur; -1 when the shape is not covered. */
  int vksift_hip_seed_direct(const uint8_t *src, uint32_t sw, uint32_t sh, uint64_t src_img_stride, vksift_hip_Plane dst, const float *taps, uint32_t ntaps,
                             uint32_t batch, vksift_hip_stream s);

  /* vkCmdBlitImage(NEAREST) of sift_detector.c:1003-1034: dst(x,y) = src(floor((x+.5)*sw/dw), ...). */
  int vksift_hip_downsample(vksift_hip_Plane src, vksift_hip_Plane dst, uint32_t batch, vksift_hip_stream s);

  /* The scale-space of n_oct consecutive (trailing) octaves in ONE launch, one workgroup per image, planes held in LDS:
   * layers[o * n_layers + l] = layer l of octave o; layer 0 of octave 0 of the run is the input (already in memory), every other plane is
   * written: layer l = blur(layer l - 1, taps[l]) (sift_detector.c:927-1001), layer 0 of the next octave = nearest 2:1 of layer S
   * (:1003-1034). taps: n_layers rows of VKSIFT_HIP_MAX_TAPS. Bit-identical to the vksift_hip_blur / vksift_hip_downsample sequence.
   * -1 when the planes are not covered (fp16, width or pitch not a multiple of 4, a base that is not 16-byte aligned, sides below 8, too
   * large for the LDS) or a layer's tap count exceeds the shortest side of any plane of the run (one mirror reflection must cover the radius). */
  int vksift_hip_octave_chain(const vksift_hip_Plane *layers, uint32_t n_oct, uint32_t n_layers, uint32_t S, const float *taps, const uint32_t *ntaps,
                              uint32_t batch, vksift_hip_stream s);

  /* DifferenceOfGaussian.comp:13-17 for one layer of one image: out (dense w x h, fp32) = hi - lo (rounded to binary16 for an
   * fp16 pyramid); hi == NULL: the layer lo itself, widened. Only the debug downloads use it — the detection path never
   * materialises a DoG plane. */
  int vksift_hip_dog_plane(const float *lo, const float *hi, uint32_t w, uint32_t h, uint32_t pitch, uint32_t fp16, float *out_dense, vksift_hip_stream s);

  /* ------------------------------------------------------------------ keypoints */
  typedef struct
  {
    float *gauss;        /* Gaussian layer 0 of image 0 of this octave (S+3 layers; DoG layer s = layer s+1 - layer s) */
    uint32_t fp16;       /* the layers hold binary16 texels (see vksift_hip_Plane); strides stay in texels */
    uint32_t w, h, pitch;
    uint64_t plane_stride; /* floats between layers */
    uint64_t img_stride;   /* floats between images */
    uint32_t S;            /* scales per octave */
    int32_t octave_idx;    /* octave index minus 1 when up-sampling (sift_detector.c:1134) */
    float seed_sigma;
    float dog_threshold;   /* intensity_threshold / S (sift_detector.c:1136) */
    float edge_limit;      /* (edge+1)^2/edge (ExtractKeypoints.comp:203) */
    /* SIFT buffer section of this octave for image 0; image b uses + b*feat_img_stride bytes */
    uint8_t *feats;        /* vksift_Feature records */
    uint64_t feat_img_stride; /* bytes */
    uint32_t cap;          /* section capacity (max_nb_feat) */
    uint32_t *found;       /* per image: counter of this octave, image b at found[b*found_img_stride] */
    uint32_t found_img_stride;
    /* scratch, per image: */
    uint64_t *seg_mask;    /* S*h*nseg words, nseg = ceil(w/64) */
    uint32_t *seg_off;     /* same count */
    uint64_t seg_img_stride; /* elements between images (both arrays); must equal S*h*nseg (contiguous batch) */
    uint32_t *cand_xy;     /* cand_cap packed candidate coordinates */
    uint32_t *cand_flag;   /* cand_cap accept flags */
    uint32_t *cand_n;      /* one counter per image (consecutive) */
    uint64_t cand_img_stride; /* elements between images (cand_xy, cand_flag) */
    uint32_t cand_cap;
    float *ori_ang;        /* cap*VKSIFT_HIP_MAX_ORI floats */
    uint32_t *ori_cnt;     /* cap */
    uint64_t ori_img_stride; /* in keypoints */
    uint32_t max_ori;      /* max_nb_orientation_per_keypoint (0 = unlimited) */
    uint32_t use_vlfeat;
    const float *desc_fp_tab; /* fixed-point multipliers indexed by R/2 (ComputeDescriptors.comp:116-124) */
    uint32_t desc_fp_tab_len;
    uint32_t scan_reverse;    /* dispatch-order hint of the streaming extrema scan, like vksift_hip_Plane::reverse: set when the last
                               * blur launch of the octave ran forward, so that the scan starts on the planes written last */
    uint32_t masks_cleared;   /* the caller has cleared seg_mask for this launch itself (vksift_hip_clear_segment_masks, e.g. on another
                               * stream, off the critical path): vksift_hip_extract_keypoints_multi skips its own fill */
    uint32_t sec_index;       /* sections of the SIFT buffer in front of this octave's (vksift_hip_DenseRows); found[-sec_index .. ] are the
                               * counters of the buffer's sections in order */
  } vksift_hip_OctaveJob;

  /* The matcher's view of a freshly detected SIFT buffer, written by the descriptor launch itself (pack_BufferMemory,
   * sift_memory.c:957-1047, without a pass of its own): feature k of section o is row sum_{j<o} min(found[j], sec_cap[j]) + k of the
   * buffer's dense 128-byte descriptor rows — download order —, its shifted norm beside it, the row total in n[]; rows below 2 of a
   * buffer with fewer features are zero-filled (quirk Q6). Image b of the batch: desc + b*desc_img_stride bytes, norm + b*norm_img_stride
   * words, n[b*n_img_stride]. Every job of the call names its section (sec_index) and all jobs share the section table. */
  typedef struct
  {
    uint8_t *desc;
    uint64_t desc_img_stride;
    uint32_t *norm;
    uint64_t norm_img_stride;
    uint32_t *n;
    uint32_t n_img_stride;
    uint32_t nsec;
    uint32_t sec_cap[16];
    /* feature posting (single-image detections): the same rows as dense 164-byte RECORDS into host-mapped memory — what
     * vksift_hip_pack_features would store there — and the buffer's found_post_n section counters beside them (image b: post +
     * b*post_img_stride bytes, found_post + b*found_post_n words). NULL: off. desc / norm / n may then be NULL as well (rows not wanted). */
    uint8_t *post;
    uint64_t post_img_stride;
    uint32_t *found_post;
    uint32_t found_post_n;
  } vksift_hip_DenseRows;

  /* ExtractKeypoints.comp (sift_detector.c:1106-1189) as a deterministic, atomic-free pipeline: streaming
   * 26-neighbour test -> per-64-pixel-segment candidate ballots -> exclusive scan -> compact candidate list ->
   * dense refinement -> per-image scan + emit in raster order. found[] receives the un-clamped keypoint count.
   * scan_done (may be NULL): recorded right after the streaming scan kernel, the one bandwidth-bound launch of the stage.
   * Contract (all three entry points; tests/test_gpu_extract_launcher.py sweeps it). READ: for every image b < batch the S + 3 Gaussian layers
   * at gauss + b * img_stride + l * plane_stride texels, rows pitch texels apart; the w x h texels of every layer are finite, whatever lies
   * in the pitch padding, between layers or between images is never interpreted. Served: sides 1 .. VKSIFT_HIP_MAX_OCTAVE_SIDE (planes below
   * 3 x 3 have no interior texel and yield nothing), S = 1 .. 13, planes (pitch * h texels) below 2 GiB, pitch >= w, plane_stride >= pitch * h
   * (layers and images may be laid out in either order and with gaps). fp32 texels: any such pitch and strides, gauss 4-byte aligned. binary16
   * texels: the scan loads the texel pair (x, x + 1), x even, as one dword, so pitch, plane_stride and img_stride must be EVEN and gauss
   * 4-byte aligned. Scratch: seg_img_stride == S * h * ceil(w / 64), both for seg_mask (u64) and seg_off (u32) — the chunk counts the emit stage
   * keeps in seg_off, one word per 256 candidates, always fit: an image has at most 64 candidates per segment —; cand_cap >=
   * ceil(S * h * ceil(w / 64) / 4096) (the scan's chunk totals live in cand_flag for a while); cand_img_stride >= cand_cap. An image with more
   * candidates than cand_cap keeps the first cand_cap of them in raster order (scale, y, x) and the rest is dropped without a word: records and
   * found are then those of the kept candidates alone (S * 2 * ((w - 1) / 2) * ((h - 1) / 2) candidates are the most an octave can have).
   * WRITTEN, per image: words 0..8 of the first min(found, cap) records of the section, in raster order (scale, y, x) of the candidate texel
   * they were refined from, orientation = 0; found[b * found_img_stride], un-clamped, also when the image has no candidate at all. The scratch
   * arrays are left with unspecified contents, every write inside the first seg_img_stride * batch elements of seg_mask / seg_off, the first
   * cand_cap elements of every image's cand_xy / cand_flag and the batch words of cand_n. Nothing else: not bytes 36..163 of any record, not a
   * record at or beyond cap, not the counter of another section, not ori_ang / ori_cnt.
   * hipErrorInvalidValue and NOTHING launched (no mask is cleared either, and no job of a multi-octave call runs): a side of 0 or above
   * VKSIFT_HIP_MAX_OCTAVE_SIDE, S = 0 or S > 13, pitch < w, plane_stride < pitch * h, a plane of 2 GiB or more, a gauss pointer that is not
   * 4-byte aligned, an odd pitch, plane_stride or img_stride with binary16 texels, seg_img_stride != S * h * ceil(w / 64), cand_cap below the
   * chunk count, cand_img_stride < cand_cap. */
  int vksift_hip_extract_keypoints(const vksift_hip_OctaveJob *job, uint32_t batch, vksift_hip_stream s, vksift_hip_event scan_done);
  /* ComputeOrientation.comp (sift_detector.c:1191-1241): main orientation written in place, extra
   * orientations appended in (keypoint, bin) order; found[] updated.
   * Contract of the records (both launchers; tests/test_gpu_feature_launchers.py sweeps it). READ: for every image the first min(found, cap)
   * records of the section hold what vksift_hip_extract_keypoints can emit: 0 <= scale_x < w and 0 <= scale_y < h, scale_idx <= S + 1, a
   * finite sigma > 0 with sigma / 2^octave_idx from 0.02 to 29 (orientation windows of radius 0 .. 130, descriptor windows of radius 1 .. 257
   * texels; octave_idx -1 .. 6); the descriptor launcher also reads orientation, in [0, 2 pi]. No other field is interpreted. A window may be
   * larger than the plane and the planes may be as small as 3 x 3. WRITTEN by the orientation launcher, per image: word 7 (orientation) of
   * those records that have a histogram peak (a record without one keeps its word: quirk Q4); for every further peak of a record — up to
   * max_ori per record, 0 = all — a copy of its 9 header words with that angle at record found, found + 1, .. in (keypoint, bin) order,
   * dropped at and beyond cap; found itself, raised by the number of copies whether stored or dropped (un-clamped); and the scratch rows
   * ori_ang / ori_cnt of the first min(found, cap) records. Nothing else: not the descriptor bytes of any record, not a record at or beyond
   * cap, not the counter of another section. */
  int vksift_hip_orientations(const vksift_hip_OctaveJob *job, uint32_t batch, vksift_hip_stream s);
  /* ComputeDescriptors.comp (sift_detector.c:1243-1259).
   * READ: as above (found as the orientation launcher left it), and desc_fp_tab[min(R / 2, desc_fp_tab_len - 1)]. WRITTEN, per image: bytes
   * 36..163 (descriptor) of the first min(found, cap) records — all zero for a window without a texel of the image interior or without a
   * gradient — and, through vksift_hip_descriptors_multi_dense, the dense rows, norms, n and the posting that vksift_hip_DenseRows describes.
   * Nothing else. */
  int vksift_hip_descriptors(const vksift_hip_OctaveJob *job, uint32_t batch, vksift_hip_stream s);
  /* The same three stages for SEVERAL octaves of one detection in one chain of launches: the reference records the dispatches of
   * all octaves of a stage into one command buffer (sift_detector.c:1106-1259); here the workgroups of all octaves share one flat
   * grid per kernel (csrc/hip/multi.h), so a stage costs 1-8 launches whatever the number of octaves, and the small octaves' work
   * fills the gaps of the large one's instead of trickling through launches of their own. jobs[0..n_jobs): same batch; results are
   * identical to calling the single-octave form once per job. Any number of jobs: the list is cut into runs of at most 8 (VKSIFT_TUNE_MULTI_MAX)
   * consecutive jobs of the same S and texel type, one chain of launches per run. scan_done as above (recorded behind the last run's scan). */
  int vksift_hip_extract_keypoints_multi(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s, vksift_hip_event scan_done);
  /* the clear of the candidate-ballot masks that vksift_hip_extract_keypoints_multi starts with, on its own (see masks_cleared): zeroes the
   * seg_img_stride * batch words of every job's seg_mask and nothing else (one fill per run of jobs whose regions follow each other, never
   * the bytes between regions that do not); at most 16 jobs. A launch only skips its own clear when EVERY job of its run has masks_cleared set. */
  int vksift_hip_clear_segment_masks(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s);
  /* test entry (tests/test_gpu_descriptor_ranges.py): the in-range forms of sqrtf, '/' and x / 2 pi that the orientation and descriptor kernels
   * use (features_math.h: sqrt_inrange, div_inrange, div_2pi_inrange) against the compiler's general forms on n pseudo-random operands
   * inside their ranges (the kernel lives in features_selftest.hip, outside the production translation unit), incl. the range ends; *d_mismatches (device memory, one word) = results that differ in any bit */
  int vksift_hip_selftest_inrange(uint32_t n, uint32_t seed, uint32_t *d_mismatches, vksift_hip_stream s);
  int vksift_hip_orientations_multi(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s);
  int vksift_hip_descriptors_multi(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s);
  /* ... and the dense matcher rows of every buffer with them (dense == NULL: as above). The counters of ALL sections must be final:
   * queue it behind vksift_hip_orientations_multi of every octave of the detection. */
  int vksift_hip_descriptors_multi_dense(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, const vksift_hip_DenseRows *dense,
                                         vksift_hip_stream s);

  /* ------------------------------------------------------------------ caller-supplied keypoints (place.hip; no counterpart in the reference) */
  typedef struct
  {
    float x, y, sigma, orientation, response; /* image pixels; 20 bytes */
  } vksift_hip_Keypoint;
  /* One octave of the placement: its extent, its index (vksift_hip_OctaveJob::octave_idx) and its section of the SIFT buffer of image 0; image b
   * uses feats + b * feat_img_stride bytes and found[b * found_img_stride] */
  typedef struct
  {
    uint32_t w, h;
    int32_t octave_idx;
    uint8_t *feats;
    uint64_t feat_img_stride; /* bytes */
    uint32_t cap;             /* section capacity */
    uint32_t *found;
    uint32_t found_img_stride;
  } vksift_hip_PlaceOctave;
  /* The inverse of the last lines of the keypoint refinement: caller-supplied keypoints (x, y, sigma in image pixels) become records that
   * vksift_hip_orientations* and vksift_hip_descriptors* accept, placed in the octave sections of their image's SIFT buffer. One launch, one
   * workgroup of VKSIFT_HIP_PLACE_WG threads per image, no atomics: the order is the input order. Keypoints kp_first[b] .. kp_first[b + 1] - 1 of
   * kps belong to image b (kps, kp_first, placed: device memory; oct and sigma_steps: host tables, copied by the call).
   * All arithmetic fp32, every operation rounded once (tests/np_describe.py restates it bit for bit). Octave: the first o of 0 .. n_oct - 1 with
   * rel = sigma * 2^-octave_idx[o] < sigma_steps[S], the last octave if there is none; scale_idx = the number of j in 0 .. S with rel >=
   * sigma_steps[j] (0 .. S, up to S + 1 in the last octave); comparisons only. With sigma_steps[j] = (float)(seed_sigma * 2^((j + 0.5) / S)) this
   * inverts sigma = seed_sigma * 2^(ss / S) * 2^octave_idx, scale_idx = round(ss). scale_x = x * 2^-octave_idx, scale_y likewise: the exact inverse
   * of x = scale_x * 2^octave_idx. Admissible: x, y, sigma finite; 0.02 <= rel <= 29; 0 <= scale_x < w[o] and 0 <= scale_y < h[o]; with
   * keep_orientation, 0 <= orientation <= 2 pi. An inadmissible keypoint produces nothing.
   * WRITTEN, per image: words 0..8 {x, y (the supplied bits), scale_x, scale_y, scale_idx, octave_idx, sigma (the supplied bits), orientation (the
   * supplied bits with keep_orientation, else 0), intensity = response (the supplied bits)} of records 0, 1, .. of the keypoint's section in input
   * order, those at and beyond cap dropped; found[o] = the un-clamped number of admissible keypoints of octave o, for every octave, zeros
   * included; placed[b] = the records stored. Nothing else: not bytes 36..163 of any record, not a record at or beyond cap.
   * hipErrorInvalidValue, nothing launched: n_oct 0 or above 16, S 0 or above 13, oct, sigma_steps, kp_first or placed NULL, a section or a counter pointer
   * that is NULL, a section or feat_img_stride that is not a multiple of 4, an octave_idx outside -31 .. 31. batch 0 returns 0 and launches nothing. */
#define VKSIFT_HIP_PLACE_WG 256u
  int vksift_hip_place_keypoints(const vksift_hip_Keypoint *kps, const uint32_t *kp_first, const vksift_hip_PlaceOctave *oct, uint32_t n_oct,
                                 const float *sigma_steps, uint32_t S, uint32_t keep_orientation, uint32_t batch, uint32_t *placed, vksift_hip_stream s);

  /* ------------------------------------------------------------------ matcher */
  /* vksift_Feature records (stride 164 B) -> dense 128-byte descriptor rows. Replaces the section packing of sift_memory.c:957-1047 as the
   * matcher's input preparation.
   * Contract of the record-moving launches (this one, vksift_hip_shifted_norms, _gather_sections, _pack_features, _filter_matches,
   * _gather_correspondences, _gather_xy; tests/test_gpu_record_launchers.py sweeps it against tests/np_records.py, byte for byte).
   * READ: bytes 36..163 of the n records at feats (4-byte aligned; a record base need not be 16-byte aligned). WRITTEN: the n * 128 bytes at
   * desc (4-byte aligned; the matcher wants 16). Nothing else; n == 0 returns 0 and launches nothing. */
  int vksift_hip_gather_descriptors(const uint8_t *feats, uint32_t n, uint8_t *desc, vksift_hip_stream s);
  /* Get2NearestNeighbors.comp (sift_matcher.c:246-279) on dense descriptor matrices in HBM, as an exact int8
   * MFMA contraction with a fused top-2 epilogue. desc_a: na rows, desc_b: nb >= 2 rows (callers pad, quirk Q6).
   * norm_scratch: scratch_u32 words of scratch, at least vksift_hip_match_scratch_u32(na, nb) (= the macro
   * VKSIFT_HIP_MATCH_SCRATCH_U32; the call returns hipErrorInvalidValue WITHOUT launching anything when it is given less: the
   * requirement grew between ABI versions 4 and 5, and a buffer sized by an old formula must fail loudly, not be overrun).
   * matches: na records of 20 B {idx_a = a_index_base + row, idx_b1,
   * idx_b2, dist1, dist2}; B rows are scanned in index order, so sharding A rows over GPUs (a_index_base =
   * shard offset) gives bit-identical results to a single call. */
  size_t vksift_hip_match_scratch_u32(uint32_t na, uint32_t nb);
  int vksift_hip_match_2nn_desc(const uint8_t *desc_a, uint32_t na, uint32_t a_index_base, const uint8_t *desc_b, uint32_t nb, uint32_t *norm_scratch,
                                size_t scratch_u32, uint8_t *matches, vksift_hip_stream s);
  /* The two halves of vksift_hip_match_2nn_desc, for callers that overlap the pre-pass of A with the arrival of B (the sharded
   * matcher: RCCL all-gather of B): norms[i] = sum over the 128 bytes of (byte - 128)^2; scratch:
   * scratch_u32 >= vksift_hip_match_scratch_u32(na, nb) - na - nb words (= 72 + 513 na; checked like above. Up to ABI version 7 the figure was one
   * na smaller, and the cell scan wrote past it: its row list takes up to na + 4 words in front of the 512 na words of the rows' lists).
   * vksift_hip_match_2nn_prenormed (tests/test_gpu_match_launchers.py sweeps the three matcher entries against tests/np_match.py, byte for byte) —
   * READ: the na rows of 128 bytes at desc_a and the nb >= 2 rows at desc_b (16-byte aligned), norm_a[0..na), norm_b[0..nb). WRITTEN: the na records
   * of 20 bytes at matches (4-byte aligned), idx_a = a_index_base + row modulo 2^32; scratch[0..scratch_u32) holds unspecified values afterwards
   * (16-byte aligned; it needs no initialisation). Nothing else: not a record at or beyond na, not a word of scratch at or beyond scratch_u32.
   * vksift_hip_match_2nn_desc — the same, the norms being computed into the first na + nb words of its scratch. na == 0: both return 0 and launch
   * nothing. hipErrorInvalidValue, nothing launched: nb < 2, scratch NULL, scratch_u32 below the figure.
   * vksift_hip_shifted_norms — READ: the n rows of 128 bytes at desc (16-byte aligned: rows are loaded 16 bytes at a time). WRITTEN: norms[0..n),
   * exact (0 for a row of 128s, 128^3 for a row of zeros). Nothing else; n == 0 returns 0 and launches nothing. */
  int vksift_hip_shifted_norms(const uint8_t *desc, uint32_t n, uint32_t *norms, vksift_hip_stream s);
  int vksift_hip_match_2nn_prenormed(const uint8_t *desc_a, const uint32_t *norm_a, uint32_t na, uint32_t a_index_base, const uint8_t *desc_b,
                                     const uint32_t *norm_b, uint32_t nb, uint32_t *scratch, size_t scratch_u32, uint8_t *matches, vksift_hip_stream s);

  /* Cross-check + Lowe ratio over forward (A->B) and optional reverse (B->A, rev != NULL) 2-NN records, the CPU loop of
   * src/examples/test_sift_match.cpp:90-107 / src/perf/perf_common.cpp:123-169: keep record i iff d1/d2 < ratio and (with
   * rev) rev[idx_b1].idx_b1 == i and its own d1/d2 < ratio. n_fwd[slot*n_stride + {0,1}] = {N_A, N_B} on the device.
   * out: per slot 16-byte records {idx_a, idx_b, dist_a_b1, dist_a_b2} in increasing idx_a order, out_n[slot] their number.
   * Strides in bytes.
   * READ, per slot: {N_A, N_B} at n_fwd[slot * n_stride + 0..1]; the N_A forward records (20 bytes {idx_a, idx_b1, idx_b2, dist1, dist2}) at
   * fwd + slot * fwd_slot_stride; with rev, record idx_b1 of the reverse table at rev + slot * rev_slot_stride for every forward record that
   * passed its own test and has idx_b1 < N_B — never a reverse record at or beyond N_B. The quotient is the correctly rounded fp32 division of
   * the two stored distances, compared with `<`: a NaN quotient (0 / 0, inf / inf, a NaN distance) or an infinite one (x / 0) drops the record,
   * 0 / x keeps it, subnormal distances divide like any others. Record i of a table is row i: "rev[idx_b1].idx_b1 == i" compares with the
   * position, the output carries the stored idx_a. WRITTEN, per slot: the kept records {fwd[i].idx_a, idx_b1, dist1 bits, dist2 bits} in
   * increasing i at out + slot * out_slot_stride, and out_n[slot]. Nothing else: not a record at or beyond out_n[slot]. Every forward record
   * may survive: the CALLER provides out_slot_stride >= 16 * N_A for every slot (N_A lives on the device; the launcher cannot check it).
   * hipErrorInvalidValue, nothing launched: nslots 0; fwd, rev (when given) or out not 4-byte aligned; fwd_slot_stride, rev_slot_stride (with
   * rev) or out_slot_stride not a multiple of 4. */
  int vksift_hip_filter_matches(const uint8_t *fwd, uint64_t fwd_slot_stride, const uint8_t *rev, uint64_t rev_slot_stride, const uint32_t *n_fwd,
                                uint32_t n_stride, float ratio, uint32_t nslots, uint8_t *out, uint64_t out_slot_stride, uint32_t *out_n, vksift_hip_stream s);

  /* Asynchronous (and batched) matching pipeline used by vksift_matchFeatures / vksift_ext_matchFeaturesBatch — no
   * host round trip for the feature counts.
   * gather_sections: fills the matcher's per-buffer cache entries of the SIFT buffers buf_ids[0..nslots), nslots <= VKSIFT_HIP_GATHER_SLOTS (feats_base +
   * id*buf_stride, counters found_base + id*found_buf_stride; all buffers of one call share the section table): walks up
   * to 16 sections whose stored counts are min(found[o], sec_cap[o]) (or fixed_counts[o] when found_base is NULL), writes
   * the dense descriptor rows in download order to desc + id*desc_stride, their shifted norms to norms + id*norm_stride and
   * the row total to n_out_dev[id*n_stride]; rows below pad_rows_to are zero-filled (quirk Q6). max_rows sizes the grid and nothing else:
   * the kernel strides over the total it reads on the device, so the results do not depend on max_rows (0 and values far above the total
   * included).
   * READ, per named buffer id: found_base[id * found_buf_stride + o] for o < nsec (found_buf_stride >= nsec is the caller's to provide: the
   * launch reads nsec counters whatever the stride; no counter at or beyond nsec, no entry of sec_off / sec_cap / fixed_counts at or beyond
   * nsec), and bytes 36..163 of the stored records. WRITTEN, per named buffer — addressed by the BUFFER's id, not by the slot that names it —:
   * max(total, pad_rows_to) rows of 128 bytes at desc + id * desc_stride (rows total .. pad_rows_to - 1 all zero), as many norms at norms +
   * id * norm_stride (128^3 for a zero row), and n_out_dev[id * n_stride] = total. Nothing else: not the entry of a buffer that is not named,
   * not a row at or beyond that count, not the padding of a stride. A buffer named twice is written twice with the same bytes. nsec == 0: every
   * buffer is empty. Alignment: feats_base and buf_stride multiples of 4 (records are loaded as dwords), desc and desc_stride multiples of 16
   * (rows are stored 16 bytes at a time). hipErrorInvalidValue, nothing launched: nslots 0 or above VKSIFT_HIP_GATHER_SLOTS, nsec above 16, a
   * misaligned feats_base, buf_stride, desc or desc_stride.
   * match_2nn_async (nslots <= VKSIFT_HIP_MATCH_SLOTS): slot i matches cache entry ids_a[i] against ids_b[i]; it first writes {N_A, N_B} of every slot to
   * n_dev[i*n_slot_stride + 0..1] (read by the kernels, the filter and the host). Strides in bytes for desc/matches and in
   * u32 elements for norms/redo/n. partial_scratch (may be NULL): 5*max_na*VKSIFT_HIP_MATCH_CHUNKS u32 used by the
   * stream-decomposed single-pair kernel (nslots == 1; without it a single pair takes the batch kernels). redo: max_na u32 per slot of row flags for the exact scalar replay.
   * max_na / max_nb: host-side bounds on the row counts of any slot (the counts themselves stay on the device); a batch whose max_nb is within the
   * packed-key kernel's range launches that kernel only — the pruning kernels' grids for larger reference sets are not queued at all. nb_exact: max_nb
   * is the largest N_B itself (every count has reached the host), not a capacity bound: only then are the pruning kernels queued for the slots
   * beyond the packed-key range; with a mere bound the packed-key kernel serves every slot of the batch whatever its N_B (exact for any size: it
   * walks B in super-chunks of 4096 columns; beyond 32 768 rows the pruning kernel is the faster one, which is all the regime was for).
   * READ, per slot i: cache_n[ids_a[i]], cache_n[ids_b[i]] (cache_n is dense: one word per entry); rows [0, N_A) of entry ids_a[i] and rows [0, max(N_B, 2))
   * of entry ids_b[i] (at cache_desc + id * cache_desc_stride, 16-byte aligned, stride a multiple of 16) with their norms (cache_norm + id *
   * cache_norm_stride words): an entry of fewer than two rows holds zero rows with norm 128^3 up to row 2, as vksift_hip_gather_sections leaves it
   * (quirk Q6). Never a row or a norm at or beyond that, whatever it holds; entries in any order, one entry as A and B, one entry in several slots.
   * WRITTEN, per slot: n_dev[i * n_slot_stride + 0..1] = {N_A, N_B} — the counts as stored, N_B not raised to two —, and, unless max_na is 0, the N_A
   * records at matches + i * match_slot_stride (a multiple of 4) as vksift_hip_match_2nn_prenormed writes them with a_index_base 0. redo[i *
   * redo_slot_stride + 0 .. max_na) and partial_scratch[0 .. 5 * max_na * VKSIFT_HIP_MATCH_CHUNKS) hold unspecified values afterwards. Nothing else: not a
   * record at or beyond N_A, not the padding of a stride, not the other words of an n_slot_stride. max_na >= every N_A is the CALLER's to provide (the
   * grids and the scratch are sized by it); a larger value gives the same bytes; max_na == 0 writes the count words only. hipErrorInvalidValue, nothing
   * launched: nslots 0 or above VKSIFT_HIP_MATCH_SLOTS. */
  /* Download packing for a batch of up to 64 SIFT buffers that share one section table (the buffers of one batched detection):
   * slot i copies the stored records of buffer buf_ids[i] — sections in order, min(found, capacity) each, the order
   * vksift_downloadFeatures returns (sift_memory.c:957-1047, 1160-1196) — as dense 164-byte records to out + out_rows[i] * 164.
   * The host then reads every buffer of the detection with one device-to-host copy instead of one per section and buffer.
   * found_post (or NULL): a host-mapped mirror of found_base; the counters of the packed buffers are stored there as well.
   * READ, per slot: the nsec counters and the stored records of buffer buf_ids[i], as vksift_hip_gather_sections reads them (found_buf_stride
   * >= nsec is the caller's to provide). WRITTEN: the total_i stored records at out + out_rows[i] * 164 — out_rows in any order, with or
   * without room between the slots' runs, which stays untouched — and, with found_post, found_post[id * found_buf_stride + k] =
   * found_base[id * found_buf_stride + k] for all k < found_buf_stride of the NAMED buffers only. Nothing else. max_rows sizes the grid and
   * nothing else (an understated value, 0 included, gives the same bytes). hipErrorInvalidValue, nothing launched: nslots 0 or above 64, nsec
   * above 16, found_post with found_buf_stride above 256, feats_base, buf_stride or out not a multiple of 4. */
  int vksift_hip_pack_features(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, const uint32_t *out_rows, uint32_t nslots, uint32_t nsec,
                               const uint32_t *sec_off, const uint32_t *sec_cap, const uint32_t *found_base, uint32_t found_buf_stride, uint8_t *out,
                               uint32_t max_rows, uint32_t *found_post, vksift_hip_stream s);
  int vksift_hip_gather_sections(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec,
                                 const uint32_t *sec_off, const uint32_t *sec_cap, const uint32_t *fixed_counts, const uint32_t *found_base,
                                 uint32_t found_buf_stride, uint32_t max_rows, uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_stride,
                                 uint32_t *norms, uint64_t norm_stride, uint32_t *n_out_dev, uint32_t n_stride, vksift_hip_stream s);
  /* The feature budget (strongest.hip): every SIFT buffer buf_ids[0..nslots), nslots <= VKSIFT_HIP_GATHER_SLOTS, keeps its max_features strongest
   * records, in place; one launch, one 1024-thread workgroup per buffer, all buffers of the call share the section table (named as for
   * vksift_hip_gather_sections: the counters are found_base + id*found_buf_stride, or fixed_counts for uploaded buffers — exactly one of the two).
   * Rows are numbered in download order. key(row) = the record's intensity word (byte 32) with the sign bit cleared, compared as an unsigned
   * integer (|DoG response| for every finite value; -0 equals +0, infinities rank above finite values, NaN patterns above those; no float
   * comparison). The first min(total, max_features) rows by (key descending, row ascending) are kept; they stay in their section, keep their
   * order and move to its front: section o then holds its kept[o] rows from record sec_off[o] on. The orientations of one keypoint are
   * separate records with equal keys: a tie at the threshold is broken by row, so the budget may keep some of them and not the others.
   * READ, per named buffer id: its nsec counters (or fixed_counts[o], o < nsec) and its stored records. WRITTEN, per named buffer whose total
   * exceeds max_features: records sec_off[o] .. sec_off[o] + kept[o] - 1 of every section (the kept records); found_base[id*found_buf_stride +
   * o] = kept[o] for o < nsec, and the same words of found_post (or NULL: a host-mapped mirror of found_base, stored by the kernel itself)
   * when counters are given; with desc != NULL the buffer's matcher-cache entry as vksift_hip_gather_sections would write it for the selected
   * buffer (max(max_features, pad_rows_to) rows at desc + id*desc_stride, as many norms at norms + id*norm_stride words, n_out_dev[id*n_stride] =
   * max_features). The records of a section from its new count up to its old stored count hold unspecified bytes afterwards (old records or
   * kept ones). Nothing else; of a buffer whose total is at most max_features NOTHING is written: not its records, not a counter (one above
   * its capacity stays), not its cache entry. With fixed_counts no counter is written: the caller knows the new total, min(total, max_features).
   * A buffer must not be named twice. Alignment: feats_base and buf_stride multiples of 4, desc and desc_stride multiples of 16.
   * hipErrorInvalidValue, nothing launched: nslots 0 or above VKSIFT_HIP_GATHER_SLOTS, nsec above 16, max_features 0, a misaligned feats_base,
   * buf_stride, desc or desc_stride, desc without norms or n_out_dev, found_post with found_buf_stride above 256 or without found_base,
   * fixed_counts and found_base both given or both NULL. */
  int vksift_hip_keep_strongest(uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec, const uint32_t *sec_off,
                                const uint32_t *sec_cap, const uint32_t *fixed_counts, uint32_t *found_base, uint32_t found_buf_stride, uint32_t *found_post,
                                uint32_t max_features, uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_stride, uint32_t *norms, uint64_t norm_stride,
                                uint32_t *n_out_dev, uint32_t n_stride, vksift_hip_stream s);
  /* The spatially distributed feature budget (spread.hip): vksift_hip_keep_strongest with a grid rule — every argument it shares means what it
   * means there, and the launch reads, writes and leaves alone exactly what that one does (a buffer whose total is at most max_features is not
   * written at all; kept rows stay in their section, keep their order and move to its front; counters, posted mirror and cache entry likewise).
   * Which rows are kept differs. key(row) is that launch's key. x is word 0 and y word 1 of the record, as fp32; cx(row) = the number of j <
   * grid_cols - 1 with x >= col_bounds[j], cy(row) likewise from y and row_bounds, cell = cy * grid_cols + cx. Only these comparisons take place:
   * a NaN or a negative coordinate satisfies none of the usual bounds and falls into column / row 0, -0.0 compares as 0.0, no bit pattern is
   * refused, and the bounds need not be monotone — the cell is the count of satisfied comparisons whatever they are. With C = grid_cols *
   * grid_rows and q = max_features / C: in every cell the first min(n_cell, q) rows of the cell by (key descending, row ascending) are kept; among
   * the rows these leave, the first max_features - (rows kept so far) by (key descending, row ascending) are kept too. Exactly max_features rows:
   * it is a total, not a number per cell. A 1 x 1 grid, and any grid with max_features < C, is vksift_hip_keep_strongest byte for byte; a second
   * launch with the same arguments changes nothing. tests/np_spread.py restates the rule.
   * col_bounds / row_bounds: HOST pointers to grid_cols - 1 / grid_rows - 1 floats, copied into the kernel's arguments by this call; NULL is
   * accepted where the count is 1. One 1024-thread workgroup per buffer, no atomics on global memory.
   * hipErrorInvalidValue, nothing launched: whatever vksift_hip_keep_strongest refuses, grid_cols or grid_rows 0 or above 16, a NULL bounds pointer
   * with a count above 1. */
  int vksift_hip_keep_grid(uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec, const uint32_t *sec_off,
                           const uint32_t *sec_cap, const uint32_t *fixed_counts, uint32_t *found_base, uint32_t found_buf_stride, uint32_t *found_post,
                           uint32_t max_features, uint32_t grid_cols, uint32_t grid_rows, const float *col_bounds, const float *row_bounds,
                           uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_stride, uint32_t *norms, uint64_t norm_stride, uint32_t *n_out_dev,
                           uint32_t n_stride, vksift_hip_stream s);
  /* RootSIFT descriptors (rootsift.hip): the 128 descriptor bytes of every stored record of the SIFT buffers buf_ids[0..nslots), nslots <=
   * VKSIFT_HIP_GATHER_SLOTS, are converted in place; one launch, all buffers of the call share the section table (named as for
   * vksift_hip_gather_sections: the counters are found_base + id*found_buf_stride, or fixed_counts for uploaded buffers — exactly one of the two).
   * A row d[0..127] with s = the sum of its bytes: s == 0 leaves it all zero; otherwise out[i] = min(255, r), r the integer with
   * (2r - 1)^2 s <= 2^20 d[i] < (2r + 1)^2 s — 512 sqrt(d[i] / s) rounded half up, taken exactly (integer arithmetic decides, not a float
   * rounding); out[i] == 0 iff d[i] == 0. tests/np_rootsift.py restates it. The launch converts whatever the rows hold: a second launch
   * converts a second time. max_rows sizes the grid and nothing else (0 and values far above the total give the same bytes).
   * READ, per named buffer id: its nsec counters (or fixed_counts[o], o < nsec), as vksift_hip_gather_sections reads them, and bytes 36..163 of
   * its stored records. WRITTEN, per named buffer: bytes 36..163 of its stored records; with desc != NULL the buffer's matcher-cache entry
   * exactly as vksift_hip_gather_sections would write it for the converted buffer (max(total, pad_rows_to) rows of 128 bytes at desc +
   * id*desc_stride, rows total .. pad_rows_to - 1 all zero; as many norms at norms + id*norm_stride words, 128^3 for a zero row;
   * n_out_dev[id*n_stride] = total), addressed by the BUFFER's id. Nothing else: not a record at or beyond a section's stored count, not one of
   * the nine head words of a record (the feature budget's key included), not a counter, not the gap between two buffers, not the entry of a
   * buffer that is not named, not a cache row at or beyond that count, not the padding of a stride; without desc, pad_rows_to, norms and
   * n_out_dev are not looked at. A buffer must not be named twice (it would be converted twice, by workgroups that do not wait for each
   * other). nsec == 0: every buffer is empty. Alignment: feats_base and buf_stride multiples of 4 (descriptors are loaded and stored as dwords),
   * desc and desc_stride multiples of 16 (rows are stored 16 bytes at a time). hipErrorInvalidValue, nothing launched: nslots 0 or above
   * VKSIFT_HIP_GATHER_SLOTS, nsec above 16, a misaligned feats_base, buf_stride, desc or desc_stride, desc without norms or n_out_dev,
   * fixed_counts and found_base both given or both NULL. */
  int vksift_hip_root_descriptors(uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec, const uint32_t *sec_off,
                                  const uint32_t *sec_cap, const uint32_t *fixed_counts, const uint32_t *found_base, uint32_t found_buf_stride,
                                  uint32_t max_rows, uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_stride, uint32_t *norms, uint64_t norm_stride,
                                  uint32_t *n_out_dev, uint32_t n_stride, vksift_hip_stream s);
  int vksift_hip_match_2nn_async(const uint8_t *cache_desc, const uint32_t *cache_norm, const uint32_t *cache_n, const uint32_t *ids_a, const uint32_t *ids_b,
                                 uint32_t max_na, uint32_t max_nb, uint32_t nb_exact, uint32_t *redo, uint32_t *n_dev, uint8_t *matches, uint32_t nslots, uint64_t cache_desc_stride,
                                 uint64_t cache_norm_stride, uint64_t redo_slot_stride, uint64_t match_slot_stride, uint32_t n_slot_stride,
                                 uint32_t *partial_scratch, vksift_hip_stream s);

  /* ------------------------------------------------------------------ geometric verification (verify.hip; no counterpart in the reference) */
  /* Correspondences of filtered matches: for slot i and each of its min(filtered_n[i], max_n) records {idx_a, idx_b, ..} (16 bytes, the output of
   * vksift_hip_filter_matches at filtered + i*filtered_slot_stride) the x, y fields of the two features as {xa, ya, xb, yb} at corr + i*corr_slot_stride
   * (bytes, multiple of 16). idx_a / idx_b are download-order rows; slot_tab holds four words per slot {buffer A, buffer B, layout A, layout B}: a layout word
   * with bit 31 set names a buffer of (word & 0x7fffffff) dense records (uploaded features), any other value entry `word` of layouts[], 33 words each
   * {nsec, off[16], cap[16]}, whose stored counts min(found, cap) are read on the device (found_base + buffer*found_buf_stride) like vksift_hip_gather_sections
   * does. slot_tab / layouts are read by the kernel (device or mapped pinned memory). A record naming a row its buffer does not hold gives a NaN
   * correspondence. One launch whatever nslots.
   * READ of the two tables: slot_tab[0 .. 4 nslots), and of layouts the entries the slots' layout words name — one per distinct section table, so at
   * most 2 nslots entries of 33 words: a caller that provides 2 nslots * 33 words behind `layouts` covers every list (vksift_hip_gather_xy likewise).
   * Sections of a table at or beyond found_buf_stride count as empty and their counters are not read (a found_buf_stride below nsec cuts the
   * table). A row >= the buffer's total makes THAT side's two floats the quiet NaN 0x7fc00000; the other side is gathered as usual. WRITTEN:
   * records 0 .. min(filtered_n[i], max_n) - 1 of every slot, nothing else. hipErrorInvalidValue, nothing launched: nslots 0,
   * filtered_slot_stride not a multiple of 4, corr_slot_stride not a multiple of 16, corr not 16-byte aligned. */
  int vksift_hip_gather_correspondences(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *found_base, uint32_t found_buf_stride,
                                        const uint32_t *slot_tab, const uint32_t *layouts, const uint8_t *filtered, uint64_t filtered_slot_stride,
                                        const uint32_t *filtered_n, uint32_t max_n, uint32_t nslots, float *corr, uint64_t corr_slot_stride, vksift_hip_stream s);
  /* Deterministic RANSAC homography of nslots correspondence sets in two launches. Slot i: n = min(n_dev[i*n_stride], max_n) correspondences of four floats
   * at corr + i*corr_slot_stride (bytes; 16-byte aligned). Hypothesis j of slot i samples four distinct indices from splitmix64 keyed by (seed, i, j) — the
   * same hypothesis whatever nb_hypotheses —, solves the four-point homography in closed form (fp32, coordinates up to VKSIFT_HIP_MAX_OCTAVE_SIDE) and counts the
   * correspondences with d > 0 and forward transfer error below threshold_px; the best is the largest count, ties to the lowest j. results + 52*i: float H[9]
   * (row-major, pixel coordinates, H[8] == 1), uint32 nb_matches (= n), nb_inliers, best_hypothesis, valid; masks + i*mask_slot_stride: n bytes, 1 = inlier of
   * H by the same test (their sum is nb_inliers). n < 4, a best count below 4, h22 == 0 or a non-finite entry: valid = 0 and H, nb_inliers, best_hypothesis and
   * the mask are zero. No refinement on the inliers here: H is the four-point model of the winning sample. vksift_hip_refit_homography (below) refits it
   * on its inliers, bit for bit reproducible because every sum has a fixed order; the mask is also what a caller's own refit needs.
   * tests/np_verify.py restates every output bit for bit. scratch: scratch_u32 >= vksift_hip_ransac_scratch_u32(nslots, nb_hypotheses) words, need not be
   * initialised, contents unspecified afterwards. WRITTEN: the nslots records, bytes 0 .. n-1 of every slot's mask, the scratch, nothing else (not the
   * mask bytes from n to mask_slot_stride, not a record beyond nslots; corr and n_dev are only read, n_dev only at the strided words).
   * hipErrorInvalidValue, nothing launched: nslots 0, nb_hypotheses 0 or above 65536, threshold_px not positive and finite, too little scratch, corr not
   * 16-byte aligned or corr_slot_stride not a multiple of 16, results not 4-byte aligned, strides below max_n records (corr_slot_stride < 16 max_n,
   * mask_slot_stride < max_n; only with nslots > 1: a single slot's strides address nothing and may be anything, 0 included, corr_slot_stride still a multiple of 16),
   * nslots * ceil(nb_hypotheses / 256) above 2^31 - 1. */
  size_t vksift_hip_ransac_scratch_u32(uint32_t nslots, uint32_t nb_hypotheses);
  int vksift_hip_ransac_homography(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                   uint32_t nb_hypotheses, float threshold_px, uint64_t seed, uint8_t *results, uint8_t *masks, uint64_t mask_slot_stride,
                                   uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s);
  /* The same for a fundamental matrix (same arguments, scratch, WRITTEN set and refusals; seven-point samples). Each hypothesis gives up to three models (the real roots of
   * the seven-point cubic, numbered in increasing order), model id = 4*j + root; a correspondence is an inlier when its Sampson distance is below threshold_px;
   * the best is the largest count, ties to the lowest model id. results + 56*i: float F[9] (row-major, pixel coordinates, (xb, yb, 1) F (xa, ya, 1)^T = 0, largest
   * |entry| in [1, 2)), uint32 nb_matches (= n), nb_inliers, best_hypothesis, best_root, valid; masks as above. n < 7, a best count below 8 (the seven sample
   * points fit their own model) or a non-finite model: valid = 0 and everything else zero. No rank or orientation test beyond the seven-point construction, no
   * handling of the planar degeneracy, no refit on the inliers here: F is the seven-point model of the winning sample, vksift_hip_refit_fundamental
   * (below) refits it on its inliers. tests/np_verify_f.py restates every output bit for bit. */
  int vksift_hip_ransac_fundamental(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                    uint32_t nb_hypotheses, float threshold_px, uint64_t seed, uint8_t *results, uint8_t *masks, uint64_t mask_slot_stride,
                                    uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s);

  /* ------------------------------------------------------------------ refit on the inliers (refine.hip, refine_f.hip; no counterpart in the reference) */
  /* Locally optimised refit of nslots verified homographies in one launch, one workgroup per slot, all rounds inside it. Slot i: n = min(n_dev[i*n_stride],
   * max_n) correspondences at corr + i*corr_slot_stride (as for vksift_hip_ransac_homography), the 13-word RANSAC record at start_results + 52*i and its mask
   * at start_masks + i*mask_slot_stride. A round takes the correspondences whose mask byte is 1 (fewer than four: it fails) through: conditioning of each side
   * (centroid; the power of two that brings the largest |deviation| into [1, 2), none: it fails); the inhomogeneous least-squares homography with h8 = 1 in
   * conditioned coordinates; two Gauss-Newton steps on the forward transfer error (u/d - xb)^2 + (v/d - yb)^2; each 8x8 normal system by Gauss-Jordan with the
   * pivoting of the seven-point solve (a pivot that is zero, subnormal or not finite, or a solution that is not finite: it fails); back to pixels and divided
   * by h22 (h22 == 0 or an entry not finite: it fails); all n correspondences re-scored under the PUBLISHED model in pixel coordinates with the test and the
   * threshold of vksift_hip_match_guided (t2 = (threshold_px 2^-13)^2 2^26): the refined mask is exactly what guided matching would admit for that model, and
   * reproducible from public outputs. Round r starts from the mask of round r - 1 (the first from start_masks); it is accepted iff it did not fail and counts
   * at least as many inliers as the result kept so far (the RANSAC record at first); the first round that is not accepted ends the loop. results + 52*i: float
   * H[9] (row-major, pixels, H[8] == 1), uint32 nb_matches (= n), nb_inliers, rounds (the last accepted round; 0: H and nb_inliers are the start record's and
   * the mask is the start mask byte for byte, so its ones sum to nb_inliers only if the start record was consistent with its mask; after an accepted round
   * the bytes are 0 / 1 and sum to nb_inliers), valid; nb_inliers is never below the start record's. A start record with valid == 0: the whole record and the mask are zero.
   * Every sum over correspondences has one order (thread t of 256 adds its elements t, t + 256, ... in increasing index, a fixed butterfly over the 64 lanes,
   * the four waves in order), everything is correctly rounded fp32 add / sub / mul / div, coordinates up to VKSIFT_HIP_MAX_OCTAVE_SIDE: the same inputs give the
   * same bytes on every run, tests/np_refine.py restates every output bit for bit. WRITTEN: the nslots records and bytes 0 .. n-1 of every slot of masks_out,
   * nothing else (start_results, start_masks and corr are only read; no scratch). hipErrorInvalidValue, nothing launched: nslots 0, nb_rounds 0 or above 8,
   * threshold_px not positive and finite or t2 zero or not finite, corr not 16-byte aligned or corr_slot_stride not a multiple of 16, results or start_results not 4-byte aligned,
   * strides below max_n records (nslots > 1), masks_out overlapping start_masks. */
  int vksift_hip_refit_homography(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                  const uint8_t *start_results /* the 13-word RANSAC records */, const uint8_t *start_masks, uint64_t mask_slot_stride,
                                  uint32_t nb_rounds, float threshold_px, uint8_t *results, uint8_t *masks_out, vksift_hip_stream s);
  /* The same for nslots verified fundamental matrices (refine_f.hip, kernel k_refit_f): the same arguments, chain, acceptance rule, mask handling, WRITTEN
   * set and refusals; the start record is the 14-word record of vksift_hip_ransac_fundamental at start_results + 56*i, the result at results + 52*i is float
   * F[9] (row-major, pixels, largest |entry| in [1, 2)), uint32 nb_matches, nb_inliers, rounds, valid. A round takes the correspondences whose mask byte is 1
   * (fewer than eight: it fails) through: the same conditioning; the gauge f_j = 1 at the largest |entry| (bit pattern, ties to the lowest index) of the model
   * the round starts from (the kept one: the RANSAC F at first) brought into the conditioned frame; the linear least-squares F over the monomials (X x, X y, X,
   * Y x, Y y, Y, x, y, 1); two steps reweighted by 1 / g, g the Sampson denominator of the step before (zero, subnormal or not finite on a marked
   * correspondence: it fails); each step one accumulation of 44 sums and one 8x8 Gauss-Jordan as above; two Newton steps on the determinant along the cofactor
   * matrix (rank 2 without an SVD; |C|^2 zero, subnormal or not finite: it fails); back to pixels and times the power of two that brings the largest |entry|
   * into [1, 2) (none: it fails); the re-scoring under the published model with the Sampson test and threshold of vksift_hip_match_guided. No chirality test,
   * no handling of the planar degeneracy. tests/np_refine_f.py restates every output bit for bit. */
  int vksift_hip_refit_fundamental(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                   const uint8_t *start_results /* the 14-word RANSAC records */, const uint8_t *start_masks, uint64_t mask_slot_stride,
                                   uint32_t nb_rounds, float threshold_px, uint8_t *results, uint8_t *masks_out, vksift_hip_stream s);

  /* ------------------------------------------------------------------ guided matching (guided.hip; no counterpart in the reference) */
#define VKSIFT_HIP_GUIDE_HOMOGRAPHY 0u
#define VKSIFT_HIP_GUIDE_FUNDAMENTAL 1u
  /* {x, y} of every stored row of both buffers of every slot, in download order: side t (0 = A, 1 = B) of slot i as dense float2 at
   * xy + (2*i + t) * xy_side_stride * 2 floats (8-byte aligned; xy_side_stride >= max_n, rows [0, min(stored, max_n)) are written). slot_tab / layouts, the
   * section walk and the counters as for vksift_hip_gather_correspondences. One launch whatever nslots. WRITTEN: those rows, nothing else (not
   * the rows of a side from min(stored, max_n) to xy_side_stride). hipErrorInvalidValue, nothing launched: nslots 0, xy_side_stride < max_n,
   * xy not 8-byte aligned. */
  int vksift_hip_gather_xy(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *found_base, uint32_t found_buf_stride, const uint32_t *slot_tab,
                           const uint32_t *layouts, uint32_t max_n, uint32_t nslots, float *xy, uint64_t xy_side_stride, vksift_hip_stream s);
  /* Guided matching of nslots pairs in two or three launches (forward sweep, reverse sweep with cross_check, decision). Slot i: the features of A are the
   * N_A = min(n_dev[i*n_stride], max_n) rows of cache entry slot_tab[i*slot_tab_stride] (dense 128-byte rows at cache_desc + entry*cache_desc_stride bytes, their
   * shifted norms sum (byte - 128)^2 at cache_norm + entry*cache_norm_stride words: what vksift_hip_gather_sections / vksift_hip_shifted_norms write), the
   * features of B the N_B = min(n_dev[i*n_stride + 1], max_n) rows of entry slot_tab[i*slot_tab_stride + 1]; their coordinates as vksift_hip_gather_xy lays them
   * out; the model nine floats at models + i*model_stride (row-major, pixel coordinates, the convention of vksift_ext_getHomography / vksift_ext_getFundamental)
   * and the word valid[i*valid_stride] (0: the slot yields no record). slot_tab, models and valid are read by the kernels (device or mapped pinned memory).
   * (a, b) is admissible under a homography iff, with (u, v, d) = M (xa, ya, 1), d > 0 and (u - xb d)^2 + (v - yb d)^2 < (d d) t2; under a fundamental matrix
   * iff, with l = M (xa, ya, 1), m = M^T (xb, yb, 1) and r = (xb, yb, 1) l, r r < t2 ((l0 l0 + l1 l1) + (m0 m0 + m1 m1)) — correctly rounded fp32 add / sub / mul
   * in this order on unscaled pixels; t2 is the squared threshold in pixels. Forward record of a: the smallest and the second smallest key (d2 << 32 | b) over the
   * admissible b (d2: the exact integer squared descriptor distance; ties to the lowest index; no padding rows, none of the plain matcher's quirks), dist =
   * sqrtf(d2), dist2 = +inf with a single candidate; the reverse record of b likewise over the admissible a (the same relation, the model is not inverted).
   * (a, b1(a)) is kept iff dist1 <= max_distance, dist1 / dist2 < ratio and, with cross_check, a1(b1(a)) == a and the reverse record passes its own ratio test.
   * out + i*out_slot_stride (bytes): 16-byte records {idx_a, idx_b, dist1, dist2} in increasing idx_a, out_n[i] their number. tests/np_guided.py restates every
   * record bit for bit. scratch: scratch_u32 >= vksift_hip_guided_scratch_u32(nslots, max_n) words, 8-byte aligned, need not be initialised.
   * hipErrorInvalidValue, nothing launched: unknown model_kind, t2 not positive and finite, ratio or max_distance not greater than 0 (+inf is a max_distance),
   * too little scratch, a stride below max_n rows (records, norms, coordinates, output), slot_tab_stride or n_stride below 2, model_stride below 9,
   * valid_stride 0, max_n above 2^24, nslots 0 or above 65535, cache_desc not 16-byte aligned or cache_desc_stride not a multiple of 16, xy or scratch not
   * 8-byte aligned, out not 4-byte aligned or out_slot_stride not a multiple of 4. WRITTEN: records 0 .. out_n[i]-1 of every slot of out, the nslots words
   * of out_n, the scratch (not the part of a slot whose valid word is 0: nslots * max_n * 8 words, slot i's at scratch + i * max_n * 8), nothing else. */
  size_t vksift_hip_guided_scratch_u32(uint32_t nslots, uint32_t max_n);
  int vksift_hip_match_guided(const uint8_t *cache_desc, uint64_t cache_desc_stride, const uint32_t *cache_norm, uint64_t cache_norm_stride, const uint32_t *slot_tab,
                              uint32_t slot_tab_stride, const float *xy, uint64_t xy_side_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n,
                              const float *models, uint32_t model_stride, const uint32_t *valid, uint32_t valid_stride, uint32_t model_kind, float t2, float ratio,
                              float max_distance, uint32_t cross_check, uint32_t nslots, uint8_t *out, uint64_t out_slot_stride, uint32_t *out_n, uint32_t *scratch,
                              size_t scratch_u32, vksift_hip_stream s);

  /* ------------------------------------------------------------------ feature tracks (tracks.hip; no counterpart in the reference) */
  /* The connected components of the graph over the stored rows of nbufs SIFT buffers whose edges are the records of nslots pairs. buf_tab: two words per
   * participating buffer, in increasing gpu_buffer_id — {gpu_buffer_id, index into rows_dev of the word that holds its row count}; the buffer at position r
   * has rank r and min(rows_dev[that word], max_rows) stored rows; node (rank, row) has the index rank * node_stride + row, so index order is the order
   * (gpu_buffer_id, row). slot_tab + i*slot_tab_stride: {rank of A, rank of B} of slot i. Slot i holds n = min(n_dev[i*n_stride], max_n) 16-byte records
   * {idx_a, idx_b, ...} at records + i*rec_slot_stride; record e is an edge between (rank A, idx_a) and (rank B, idx_b) iff valid == NULL or
   * valid[i*valid_stride] != 0, and masks == NULL or the byte masks[i*mask_slot_stride + e] is 1, and both ranks are below nbufs and both rows stored (the
   * library's own producers never leave a record that names a row that is not). A track is a component of at least two nodes; tracks are numbered from 0 in the
   * order of their smallest node. tracks + 16*t: {gpu_buffer_id, row} of the smallest node, length (nodes), nb_buffers (distinct buffers among them);
   * node_words[index]: the track number of every stored row, 0xFFFFFFFF without one; stats: {tracks, tracks with length > nb_buffers, sum of the lengths,
   * edges taken (edges inside one buffer, on one node and duplicates included)}. Deterministic: every output depends on the graph alone.
   * tests/np_tracks.py restates it. slot_tab, buf_tab and rows_dev are read by the launches (device-accessible memory): slot_tab
   * at the two words of each of the nslots strides, buf_tab[0 .. 2 nbufs), rows_dev at the nbufs words buf_tab names and nowhere else (its extent is the
   * caller's: the launch's own scalars do not bound it). scratch: scratch_u32 >=
   * vksift_hip_tracks_scratch_u32(nbufs, node_stride) words, 8-byte aligned, need not be initialised, contents unspecified afterwards (only the words of
   * stored rows and of the launch's blocks are touched). WRITTEN: the four words of stats, records 0 .. stats[0]-1 of tracks, node_words of the stored rows, the
   * scratch, nothing else. hipErrorInvalidValue, nothing launched: nslots, nbufs, max_n or max_rows 0, max_rows above node_stride, nbufs * node_stride above
   * 2^32 - 2, n_stride 0, slot_tab_stride below 2, valid given with valid_stride 0, records or tracks not 4-byte aligned, rec_slot_stride not a multiple of 4,
   * scratch not 8-byte aligned, with nslots > 1 a stride below max_n records (rec_slot_stride < 16 max_n, mask_slot_stride < max_n), tracks_cap (records)
   * below nbufs * max_rows / 2, too little scratch. */
  size_t vksift_hip_tracks_scratch_u32(uint32_t nbufs, uint32_t node_stride);
  int vksift_hip_build_tracks(const uint8_t *records, uint64_t rec_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, const uint8_t *masks,
                              uint64_t mask_slot_stride, const uint32_t *valid, uint32_t valid_stride, const uint32_t *slot_tab, uint32_t slot_tab_stride,
                              uint32_t nslots, const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows,
                              uint32_t *node_words, uint8_t *tracks, uint64_t tracks_cap, uint32_t *stats, uint32_t *scratch, size_t scratch_u32,
                              vksift_hip_stream s);

  /* ------------------------------------------------------------------ tracks across matching calls (track_edges.hip; no counterpart in the reference) */
  /* An edge store that outlives a matching. edges: max_edges 16-byte records {gpu_buffer_id A, row A, gpu_buffer_id B, row B}; stats: the four words {edges
   * held, edges dropped, calls, changed buffers}; row_table: one word per gpu_buffer_id below nb_buffers, 0xFFFFFFFF until a call records the buffer's row
   * count there. The caller zeroes stats and fills row_table with 0xFF bytes to empty the store. APPEND takes the records, counts, masks, valid words,
   * slot_tab, buf_tab, rows_dev and max_rows of vksift_hip_build_tracks and selects the edges that launcher would take, by the same rule (both ranks below
   * nbufs, the mask byte 1, the pair valid, both rows below min(rows_dev[word], max_rows)). With held = min(stats[0], max_edges) the edges go to positions held,
   * held + 1, ... in the order slot ascending, record ascending, as {buf_tab[2 rank A], idx_a, buf_tab[2 rank B], idx_b}; positions at or beyond max_edges are
   * not written. Afterwards stats[0] = min(held + taken, max_edges), stats[1] has grown by the edges that were not written (it stops at 2^32 - 1), stats[2] by 1.
   * For every rank r < nbufs with buf_tab[2 r] < nb_buffers (the ids of buf_tab are distinct): c = min(rows_dev[buf_tab[2 r + 1]], 2^32 - 2); a word of
   * row_table that is 0xFFFFFFFF becomes c, one that holds another count than c stays and adds 1 to stats[3]. Deterministic, no atomics, three launch phases
   * that each read the plain stores of the one before. scratch: scratch_u32 >= vksift_hip_track_edges_scratch_u32(nslots, max_n) words, need not be
   * initialised, unspecified afterwards. WRITTEN: stats, the new edges, the words of row_table that were 0xFFFFFFFF, the scratch, nothing else.
   * hipErrorInvalidValue, nothing launched: nslots, nbufs, max_n, max_rows, nb_buffers, max_edges or n_stride 0, slot_tab_stride below 2, valid given with
   * valid_stride 0, records not 4-byte or edges not 16-byte aligned, rec_slot_stride not a multiple of 4, scratch not 4-byte aligned, with nslots > 1 a stride
   * below max_n records, nslots * ceil(max_n / 256) above 2^31 - 1, too little scratch.
   *
   * BUILD FROM EDGES computes what vksift_hip_build_tracks computes — the same node numbering, node_words, track records and statistics, the same scratch
   * (vksift_hip_tracks_scratch_u32) and the same meaning of buf_tab, rows_dev, node_stride and max_rows — for the graph whose edges are records 0 ..
   * min(edge_count[0], max_edges) - 1 of edges (edge_count on the device, e.g. word 0 of the store's stats). rank_tab: nb_buffers words, the rank of each
   * gpu_buffer_id in buf_tab or 0xFFFFFFFF for a buffer that takes no part. A record is an edge iff both ids are below nb_buffers, both ranks below nbufs
   * and both rows stored; stats[3] counts those. With rows_dev = row_table the word index buf_tab[2 r + 1] is the gpu_buffer_id. One append followed by one
   * build gives the bytes vksift_hip_build_tracks gives for the same input. hipErrorInvalidValue, nothing launched: max_edges or nb_buffers 0, edges not
   * 16-byte aligned, and every refusal of vksift_hip_build_tracks that concerns nbufs, node_stride, max_rows, tracks, tracks_cap and the scratch.
   * tests/np_track_edges.py restates both. */
  size_t vksift_hip_track_edges_scratch_u32(uint32_t nslots, uint32_t max_n);
  int vksift_hip_append_track_edges(const uint8_t *records, uint64_t rec_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, const uint8_t *masks,
                                    uint64_t mask_slot_stride, const uint32_t *valid, uint32_t valid_stride, const uint32_t *slot_tab, uint32_t slot_tab_stride,
                                    uint32_t nslots, const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t max_rows, uint32_t *row_table,
                                    uint32_t nb_buffers, uint8_t *edges, uint32_t max_edges, uint32_t *stats, uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s);
  int vksift_hip_build_tracks_from_edges(const uint8_t *edges, const uint32_t *edge_count, uint32_t max_edges, const uint32_t *rank_tab, uint32_t nb_buffers,
                                         const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, uint32_t *node_words,
                                         uint8_t *tracks, uint64_t tracks_cap, uint32_t *stats, uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s);

  /* ------------------------------------------------------------------ track observations (observations.hip; no counterpart in the reference) */
  /* The observation table of the tracks vksift_hip_build_tracks left: which tracks a caller keeps, and their members with positions, grouped by track.
   * READ: node_words, tracks (the 16-byte records) and track_stats[0] (the track count, on the device: clamped to nbufs * max_rows / 2) as
   * vksift_hip_build_tracks wrote them, with the buf_tab, rows_dev, node_stride and max_rows of that call (read at the same words and nowhere else); the
   * first two floats of the stored record of every row: buffer b's records at feats_base + b*buf_stride bytes, its section counters at found_base +
   * b*found_buf_stride words, rank_layouts[r] the layout word of the buffer of rank r and layouts the section tables those words name, in the convention of
   * vksift_hip_gather_correspondences (VKSIFT_LAYOUT_DENSE | n, or the index of a table of 33 words); rank_layouts and layouts are read by the launches
   * (device or mapped pinned memory).
   * Track t is SELECTED iff length >= min_length and (max_length == 0 or length <= max_length) and (conflicts == 0 or length == nb_buffers). Selected tracks
   * keep their order: selected track m has track_ids[m] = t and the observations offsets[m] .. offsets[m+1], its members in increasing (gpu_buffer_id, row);
   * an observation is the 16 bytes {gpu_buffer_id, row, x, y}, x and y bit for bit. stats: {selected tracks M, observations, tracks that fail the length
   * test, tracks that pass it and are dropped as conflicting}; offsets[0] = 0 (with M = 0 too), offsets[M] = observations. A row the tracks know and the
   * layout does not hold (a buffer refilled since the matching) has x = y = 0. Deterministic: every output depends on the inputs alone (a stable radix sort
   * of the nodes by their track's new number; no atomics on global memory). tests/np_observations.py restates it.
   * scratch: scratch_u32 >= vksift_hip_observations_scratch_u32(nbufs, node_stride, max_rows) words, 8-byte aligned, need not be initialised, contents
   * unspecified afterwards. WRITTEN: the four words of stats, offsets[0 .. M], track_ids[0 .. M), observations 0 .. stats[1]-1, the scratch, nothing else.
   * offsets holds tracks_cap + 1 words, track_ids tracks_cap, observations obs_cap records.
   * hipErrorInvalidValue, nothing launched: nbufs or max_rows 0, max_rows above node_stride, nbufs * node_stride above 2^32 - 2 or the rows of whole
   * blocks of 2048 above 2^31 - 1, min_length below 2, max_length neither 0 nor >= min_length, conflicts above 1, tracks or feats_base not 4-byte aligned,
   * buf_stride not a multiple of 4, observations not 16-byte aligned, scratch not 8-byte aligned, tracks_cap below nbufs * max_rows / 2, obs_cap below
   * nbufs * max_rows, too little scratch. */
  size_t vksift_hip_observations_scratch_u32(uint32_t nbufs, uint32_t node_stride, uint32_t max_rows);
  int vksift_hip_track_observations(const uint32_t *node_words, const uint8_t *tracks, const uint32_t *track_stats, const uint32_t *buf_tab, uint32_t nbufs,
                                    const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, const uint8_t *feats_base, uint64_t buf_stride,
                                    const uint32_t *found_base, uint32_t found_buf_stride, const uint32_t *rank_layouts, const uint32_t *layouts,
                                    uint32_t min_length, uint32_t max_length, uint32_t conflicts, uint32_t *offsets, uint32_t *track_ids, uint64_t tracks_cap,
                                    uint8_t *observations, uint64_t obs_cap, uint32_t *stats, uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s);

  /* ------------------------------------------------------------------ triangulation (triangulate.hip; no counterpart in the reference) */
  /* The selected tracks of an observation table triangulated under caller-supplied cameras: one 32-byte point {X[3], max_sq_error, min_cos, status, steps,
   * nb_observations} per selected track (vksift_ext_Point).
   * READ: obs_stats[0] (the track count M, on the device: clamped to points_cap) and obs_stats[1] (the observation count), offsets[0 .. M] and the
   * observations offsets[m] .. offsets[m+1] of every track m < M as vksift_hip_track_observations wrote them (a track whose offsets decrease or end beyond
   * obs_stats[1] is DEGENERATE with nb_observations 0 and none of its observations is read; of a TOO_LONG track none is read either); cameras: 12 floats per
   * gpu_buffer_id, a row-major 3x4 P with (u, v, w) = P (X, Y, Z, 1), pixel (u / w, v / w); the cameras the read observations name and, where one names
   * gpu_buffer_id >= nb_cameras (its track is DEGENERATE), camera 0. t2: the squared threshold in pixels^2.
   * THE RULE, per track with members i = 0 .. n-1 in table order. fp32 add, sub, mul, div and sqrtf, each rounded once, in this order, no fmaf. "unusable":
   * zero, subnormal or not finite. n > 1024: TOO_LONG. n < 2: DEGENERATE.
   *  1 bearings: with rows m1, m2, m3 of P's left 3x3 block and a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0): b = (x (m2 x m3) + y (m3 x m1)) + (m1 x m2)
   *    per component, q = (b0 b0 + b1 b1) + b2 b2, s = 1 / sqrtf(q), b = b s; q or s unusable: DEGENERATE. min_cos = the minimum over all i < j of
   *    (bi0 bj0 + bi1 bj1) + bi2 bj2, taken on the integer key that orders floats (-0 below +0).
   *  2 linear start: per member the rows e = x P3 - P1 and y P3 - P2 (four entries, each t P3[c] - Pr[c]), q = (e0 e0 + e1 e1) + e2 e2, s = 1 / sqrtf(q),
   *    p = (e0 s, e1 s, e2 s), pr = e3 s (q or s unusable: DEGENERATE). With the two rows p, q of a member, the nine sums S00 S01 S02 S11 S12 S22 r0 r1 r2
   *    receive (pa pb + qa qb) and (pa pr + qa qr); the start solves S X = -r by Gauss-Jordan with refit.h's pivot rule: for column k the rows below are
   *    compared with row k in turn and exchanged when their |entry| (bit pattern) is strictly larger, row k times 1 / pivot, every other row r minus
   *    a[r][k] times row k; an unusable pivot or a solution entry that is not finite: DEGENERATE.
   *  3 up to two Gauss-Newton steps on the summed squared reprojection error. At X per member: u = ((P0 X + P1 Y) + P2 Z) + P3 and v, w alike; pu = u / w,
   *    pv = v / w, ru = pu - x, rv = pv - y, e2 = ru ru + rv rv, iw = 1 / w, ju[c] = (P1[c] - pu P3[c]) iw, jv[c] = (P2[c] - pv P3[c]) iw; the cost is the
   *    sum of e2, the normal equations the nine sums of the rows (ju | ru), (jv | rv) as in 2, the step d solves N d = -g, the new point is X + d. A step is
   *    accepted iff no w at X is unusable, the solve succeeds, X + d is finite and cost(X + d) <= cost(X); the first step that is not accepted ends the loop.
   *  4 scoring at the final X: max_sq_error = the largest e2 by |bit pattern| (any NaN reads 0x7fc00000); BEHIND iff some w <= 0; ERROR iff not
   *    max_sq_error < t2; ANGLE iff cos_min_angle < 1 and not min_cos < cos_min_angle. DEGENERATE and TOO_LONG points hold zeros but for status and
   *    nb_observations.
   *  5 every sum over members: a group of G = 16 lanes owns a track; lane j adds members j, j + 16, ... in increasing order to a partial sum that starts at
   *    +0; the lanes are added by the xor butterfly p + p[lane ^ off], off = 8, 4, 2, 1.
   * stats = {points M, accepted (status 0), failed (DEGENERATE or TOO_LONG), rejected (the others)}, integer counts. Deterministic: every output depends on
   * the inputs alone. No scratch, no atomics on global memory. tests/np_triangulate.py restates the rule.
   * WRITTEN: the M records of points, the four words of stats, nothing else. points holds points_cap records.
   * hipErrorInvalidValue, nothing launched: a NULL pointer, nb_cameras 0, points_cap 0 or above 2^31 - 1, t2 not positive and finite, cos_min_angle NaN,
   * offsets, obs_stats or stats not 4-byte aligned, observations, cameras or points not 16-byte aligned. */
  int vksift_hip_triangulate_tracks(const uint32_t *offsets, const uint8_t *observations, const uint32_t *obs_stats, const float *cameras, uint32_t nb_cameras,
                                    float t2, float cos_min_angle, uint8_t *points, uint64_t points_cap, uint32_t *stats, vksift_hip_stream s);

  /* ------------------------------------------------------------------ per-view index and camera refinement (cameras.hip; no counterpart in the reference) */
  /* The observation table inverted by view: the observations of every gpu_buffer_id below nb_cameras, each with the number of its selected track.
   * READ: obs_stats[0] (the track count M, on the device: clamped to tracks_cap) and obs_stats[1] (the observation count n, clamped to obs_cap),
   * offsets[0 .. M] and observations 0 .. n-1 as vksift_hip_track_observations wrote them.
   * Observation i < n is INDEXED iff its gpu_buffer_id is below nb_cameras and the search lo = 0, hi = M; while hi - lo > 1: mid = lo + (hi - lo) / 2,
   * offsets[mid] <= i ? lo = mid : hi = mid ends at a track m = lo with offsets[m] <= i < offsets[m+1] <= n (the triangulation's test of an extent; with
   * M = 0 nothing is indexed). What is not indexed is counted in nothing. view_offsets[0 .. nb_cameras] is the prefix sum of the indexed observations per
   * gpu_buffer_id (view_offsets[0] = 0, view_offsets[nb_cameras] their number); the records view_offsets[b] .. view_offsets[b+1] of view_observations
   * are the indexed observations of buffer b in table order (increasing i: increasing m, the two members of a conflicting track in one view in increasing
   * row), each the 16 bytes {point m, row, x, y} (vksift_ext_ViewObservation), x and y bit for bit. stats = {views with an observation, indexed
   * observations, the largest view, 0}. Deterministic: a stable LSD radix sort of the observation numbers by gpu_buffer_id (8-bit digits, as many as
   * nb_cameras needs), linear in obs_cap; no atomics on global memory. tests/np_cameras.py restates it.
   * scratch: scratch_u32 >= vksift_hip_views_scratch_u32(obs_cap) words, 4-byte aligned, need not be initialised, contents unspecified afterwards.
   * WRITTEN: view_offsets[0 .. nb_cameras], the indexed records of view_observations, the four words of stats, the scratch, nothing else.
   * view_observations holds obs_cap records.
   * hipErrorInvalidValue, nothing launched: a NULL pointer, nb_cameras 0 or 2^32 - 1, tracks_cap 0 or above 2^31 - 1, obs_cap 0 or its whole blocks of
   * 2048 above 2^31 - 1, offsets, obs_stats, view_offsets, stats or scratch not 4-byte aligned, observations or view_observations not 16-byte aligned, too
   * little scratch. */
  size_t vksift_hip_views_scratch_u32(uint64_t obs_cap);
  int vksift_hip_index_views(const uint32_t *offsets, const uint8_t *observations, const uint32_t *obs_stats, uint64_t tracks_cap, uint64_t obs_cap,
                             uint32_t nb_cameras, uint32_t *view_offsets, uint8_t *view_observations, uint32_t *stats, uint32_t *scratch, size_t scratch_u32,
                             vksift_hip_stream s);

  /* Every camera refined on the points of its view, the points held fixed (the motion half of resection-intersection): one 72-byte record {P[12],
   * cost_start, cost, max_sq_error, nb_observations, steps, status} per gpu_buffer_id below nb_cameras (vksift_ext_RefinedCamera).
   * READ: view_offsets, view_observations and view_stats[1] (the indexed count, on the device: clamped to obs_cap) as vksift_hip_index_views wrote them
   * (view b: its extent with view_offsets[b+1] clamped to that count and view_offsets[b] to the clamped end); the 32-byte points as
   * vksift_hip_triangulate_tracks wrote them: of every member whose point number is below points_cap the status word, and of the used ones X; cameras: 12
   * floats per gpu_buffer_id, the row-major 3x4 P of vksift_hip_triangulate_tracks; buf_tab[2 r], r < nbufs: the gpu_buffer_ids that took part in the build
   * (the table vksift_hip_build_tracks read). A buffer that is not among them is ABSENT: every word of its record is 0 but status.
   * THE RULE, per view with the members of its index range in order. fp32 add, sub, mul and div, each rounded once, in this order, no fmaf. "unusable":
   * zero, subnormal or not finite.
   *  1 a member is USED iff its point number is below points_cap and the status word of that point is 0; nb_observations counts them. Fewer than 6: TOO_FEW.
   *  2 evaluation at P, per used member with X its point: u, v, w, pu, pv, ru, rv, e2, iw, ju, jv as in step 3 of vksift_hip_triangulate_tracks; au = X x ju,
   *    av = X x jv with a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0); the rows p = (au0, au1, au2, ju0, ju1, ju2 | ru) and q alike from av, jv, rv.
   *    28 sums: cost += e2; the 21 upper entries of N row by row, N[a][b] += (pa pb + qa qb); g[a] += (pa ru + qa rv). Flags: some w unusable; some
   *    w <= 0. max_e2 = the largest e2 by |bit pattern|. The cost at the input camera cannot be computed (DEGENERATE) iff some w is unusable there or the
   *    cost is not finite.
   *  3 a step: N d = -g (N filled symmetrically, the right-hand side -g[a]) by the 6x7 Gauss-Jordan with refit.h's pivot rule — for column k the rows below
   *    compared with row k in turn and exchanged when their |entry| (bit pattern) is strictly larger, row k times 1 / pivot, every other row r minus a[r][k]
   *    times row k; an unusable pivot or a solution entry that is not finite fails. omega = d[0..2], tau = d[3..5]; a = 0.5 omega, b = 2 a,
   *    q = (a0 a0 + a1 a1) + a2 a2, s = 1 / (1 + q), t = 1 - q; the Cayley rotation C[i][i] = (t + b[i] a[i]) s, C[0][1] = (b0 a1 - b2) s,
   *    C[0][2] = (b0 a2 + b1) s, C[1][0] = (b1 a0 + b2) s, C[1][2] = (b1 a2 - b0) s, C[2][0] = (b2 a0 - b1) s, C[2][1] = (b2 a1 + b0) s; P' = P [[C, tau],
   *    [0, 1]]: P'[r][c] = (P[r][0] C[0][c] + P[r][1] C[1][c]) + P[r][2] C[2][c] for c < 3 and P'[r][3] = ((P[r][0] tau0 + P[r][1] tau1) + P[r][2] tau2) +
   *    P[r][3]. The step is accepted iff no w at P is unusable, the solve succeeds, every entry of P' is finite and cost(P') <= cost(P); the first step that is
   *    not accepted ends the loop; at most nb_steps steps.
   *  4 every sum over members: a workgroup of 256 lanes owns a view; lane j visits positions j, j + 256, ... of the view's range in increasing order and adds
   *    the used ones to partial sums that start at +0; the 64 lanes of a wave are added by the xor butterfly p + p[lane ^ off], off = 32 .. 1, the four
   *    waves as ((w0 + w1) + w2) + w3 (refit.h's block sum). The 256 is part of the rule.
   *  5 the record: P the final camera (the input camera where no step was accepted), cost_start and cost the cost at the input and at the final camera,
   *    max_sq_error = max_e2 at the final camera (any NaN reads 0x7fc00000), steps the accepted steps, status BEHIND iff some w <= 0 at the final camera.
   *    TOO_FEW and DEGENERATE records hold the input camera and nb_observations; the costs, max_sq_error and steps are 0 and no other flag is set.
   * stats = {views (not ABSENT), refined (steps > 0), unchanged (neither TOO_FEW nor DEGENERATE, no step), failed (TOO_FEW or DEGENERATE)}. Deterministic:
   * every output depends on the inputs alone. No scratch, no atomics on global memory. tests/np_cameras.py restates the rule.
   * WRITTEN: the nb_cameras records of refined, the four words of stats, nothing else.
   * hipErrorInvalidValue, nothing launched: a NULL pointer, nb_cameras 0 or above 2^31 - 1, nbufs 0, obs_cap or points_cap 0 or above 2^31 - 1, nb_steps 0
   * or above 8, view_offsets, view_stats, buf_tab, refined or stats not 4-byte aligned, view_observations, points or cameras not 16-byte aligned. */
  int vksift_hip_refine_cameras(const uint32_t *view_offsets, const uint8_t *view_observations, const uint32_t *view_stats, uint64_t obs_cap,
                                const uint8_t *points, uint64_t points_cap, const float *cameras, uint32_t nb_cameras, const uint32_t *buf_tab, uint32_t nbufs,
                                uint32_t nb_steps, uint8_t *refined, uint32_t *stats, vksift_hip_stream s);

#ifdef __cplusplus
}
#endif
#endif /* VKSIFT_HIP_H */
