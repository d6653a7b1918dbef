/*
 * vksift_internal.h — private definitions shared by the host translation units behind the vksift_* C API
 * (vksift_api.c, vksift_instance.c, vksift_mem.c, vksift_detect.c, vksift_stage.c, vksift_defer.c, vksift_buffers.c, vksift_match.c, vksift_verify.c, vksift_refine.c, vksift_guided.c, vksift_tracks.c, vksift_observations.c, vksift_triangulate.c, vksift_cameras.c, vksift_track_edges.c, vksift_strongest.c, vksift_rootsift.c, vksift_runs.c, vksift_describe.c, vksift_pairs.c, vksift_ext.c).
 * Nothing here is part of the public ABI; every function is hidden from the shared library's export table.
 */
#ifndef VKSIFT_INTERNAL_H
#define VKSIFT_INTERNAL_H

#include "vksift_ext.h"
#include "vksift_hip.h"
#include "hip/records.h" /* the record and section-table constants */
#include "vksift_hostmath.h"
#include "vksift_log.h"
#include "vksift_runs.h" /* BufferInfo, the layout runs, VKSIFT_INTERNAL */
#include "vulkansift/vulkansift.h"

#include <assert.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>


#define LOG_TAG "VulkanSift"

#define VKSIFT_DL_BATCH_MIN 8u
#define VKSIFT_DL_CHUNKS 8u
#define VKSIFT_UP_GROUPS 8u
#define VKSIFT_FORK_MAX_COUNT 4u /* forked scale-space (and the LDS chain): detections of at most this many images */
#define FEAT_BYTES 164u
#define MATCH_BYTES 20u
#define PITCH_ALIGN 64u
#define DESC_FP_TAB_MAX 1024u

/* One slot per detection in flight. A caller that pipelines (detection N+1 queued while it downloads the results of detection N,
 * the way vksift_isBufferAvailable is meant to be used) waits for the detection that filled the buffer it reads, not for the
 * latest one. The instance stream is in-order: a later detection's completion implies every earlier one's. */
#define VKSIFT_DETECT_RING 4
typedef struct
{
  vksift_hip_event ev;
  uint64_t seq;
  uint32_t first, count; /* SIFT buffers it filled */
} DetectSlot;

typedef struct
{
  uint32_t n_oct;
  uint32_t w[VKSIFT_MAX_OCTAVES], h[VKSIFT_MAX_OCTAVES], pitch[VKSIFT_MAX_OCTAVES];
  uint64_t plane_stride[VKSIFT_MAX_OCTAVES]; /* floats */
  uint64_t gauss_off[VKSIFT_MAX_OCTAVES];    /* floats from the image's pyramid base: S+3 Gaussian planes per octave (no DoG planes) */
  uint64_t img_floats; /* floats used by one image */
  uint64_t seg_off[VKSIFT_MAX_OCTAVES], seg_total;   /* per-octave slices of the segment scratch (elements) */
  uint64_t cand_off[VKSIFT_MAX_OCTAVES], cand_cap[VKSIFT_MAX_OCTAVES], cand_total;
} PyrLayout;

/* HIP-event stage timings of one detection (vksift_ext_setProfiling) */
/* A captured detection launch sequence (hipGraph), valid for one (resolution, batch, first buffer, input pointer) */
#define VKSIFT_GRAPH_CACHE 8
#define VKSIFT_POST_IDLE 16u
typedef struct
{
  vksift_hip_graph exec;
  uint32_t w, h, count, first_buf;
  const uint8_t *d_src;
  bool post;  /* the sequence ends with the feature posting (see h_post) */
  bool dense; /* its descriptor launch writes the buffer's matcher cache entry (captured before the first matching: it does not) */
  uint64_t stamp;
  uint64_t last_seq; /* the detection that launched it last: it may be executing until that one has completed */
} DetectGraph;

/* device scratch of one set of matching slots (slot i serves pair i of a batched call) */
typedef struct
{
  uint8_t *matches;
  uint32_t *redo, *match_n;
} MatchScratch;

/* the interval of a stage's last run under vksift_ext_setProfiling (vksift_pairs.c). One per getter: both verification models share T_VERIFY */
enum { T_MATCH, T_VERIFY, T_REFINE_H, T_REFINE_F, T_GUIDED, T_BUDGET, T_BUDGET_GRID, T_ROOTSIFT, T_TRACKS, T_OBSERVATIONS, T_TRIANGULATE, T_VIEWS, T_CAMERAS, T_ACCUMULATE, T_COUNT };
typedef struct
{
  vksift_hip_event ev[2];
  bool valid;
} StageTimer;

/* What a stage keeps for each pair of the last filtered matching (vksift_pairs.c): `words` posted words per pair (on the device, and in pinned memory
 * once the launches have passed), and a payload of `stride` bytes per pair that holds `elem` bytes for each of the n elements counted by word 0 of set
 * `counted_by`'s record (the filtered matches' own count for them and for the masks, the guided matches' for those). slots_used: the pairs that have
 * results; zero again after a new matching, and for a refit after a new verification of its model. */
enum { PR_FILTERED, PR_VERIFY_H, PR_VERIFY_F, PR_REFINE_H, PR_REFINE_F, PR_GUIDED, PR_COUNT };
typedef struct
{
  uint32_t *d_words, *h_words;
  uint8_t *d_payload;
  uint64_t stride;
  uint32_t words, elem, counted_by;
  uint32_t slots_used;
} PairResults;

/* What vksift_ext_buildTracks and vksift_ext_buildTracksAccumulated keep (vksift_tracks.c, vksift_track_edges.c): not per pair, so not a PairResults. Sized by
 * the configuration when the first build allocates it: cap_bufs participating buffers of max_nb_sift_per_buffer nodes each, cap_bufs = min(2 batch_cap,
 * sift_buffer_count), or sift_buffer_count once an accumulation has been begun (all_bufs). `valid`: the accessors have something to read; cleared by a new
 * matching (beside pair_results_invalidate). */
typedef struct
{
  uint32_t *d_node_words; /* per node (rank * max_nb_sift_per_buffer + row): its track number */
  uint8_t *d_records;     /* the vksift_ext_Track records */
  uint32_t *d_stats, *h_stats; /* the four words of vksift_ext_TrackStats, posted */
  uint32_t *d_scratch;    /* parent, length, buffer count and presence words (vksift_hip_tracks_scratch_u32) */
  size_t scratch_u32;
  uint32_t *h_tab, *d_tab; /* {rank A, rank B} per slot of batch_cap, then {gpu_buffer_id, word of d_rows} per rank of cap_bufs, then (accumulated build) the rank
                            * of every SIFT buffer: filled in pinned memory, copied to the device in front of the launches (every edge reads its pair's and
                            * its buffers' entries) */
  uint32_t *rank_of;      /* per SIFT buffer: its rank in the last build, VKSIFT_EXT_NO_TRACK for a buffer that took no part */
  uint32_t *ids;          /* per rank: the gpu_buffer_id. The participating buffers of the last build: the sides of the last pair list for a plain build, every
                           * buffer the store's calls named for an accumulated one. The stages that read the tracks keep THESE busy */
  uint32_t *count_word;   /* per rank: the word of h_rows / d_rows that holds the buffer's row count */
  const uint32_t *d_rows, *h_rows; /* the row-count words the launches read and their host mirror: d_match_n / h_match_n for a plain build, d_rows_acc /
                                    * h_rows_acc for an accumulated one */
  uint32_t *d_rows_acc, *h_rows_acc; /* per SIFT buffer: the accumulated build's copy of the store's row table, and the copy posted */
  uint32_t cap_bufs, nbufs, max_rows;
  bool all_bufs;          /* sized for sift_buffer_count buffers, not min(2 batch_cap, sift_buffer_count): since the first vksift_ext_beginTrackAccumulation */
  bool valid, tab_pending;
} TrackResults;

/* What vksift_ext_beginTrackAccumulation ... vksift_ext_buildTracksAccumulated keep (vksift_track_edges.c): the edges of every accumulated matching, on the
 * device, and one row count per SIFT buffer. Outlives matchings and builds; emptied by begin alone. */
typedef struct
{
  uint8_t *d_edges;            /* max_edges vksift_ext_TrackEdge records */
  uint32_t *d_stats, *h_stats; /* the four words of vksift_ext_TrackEdgeStats, posted by every accumulate */
  uint32_t *d_rows;            /* per SIFT buffer: the row count the first call that named it found, 0xFFFFFFFF before */
  uint32_t *d_scratch;         /* the append's block counts (vksift_hip_track_edges_scratch_u32) */
  size_t scratch_u32;
  uint32_t *h_tab, *d_tab;     /* one accumulate's {rank A, rank B} per slot of batch_cap, then {gpu_buffer_id, word of d_match_n} per buffer of the call: filled
                                * in pinned memory, copied to the device in front of the launches */
  uint32_t *rank_of;           /* per SIFT buffer: scratch of one accumulate's ranking */
  bool *named;                 /* per SIFT buffer: a call of the store has named it */
  uint32_t max_edges, max_rows, nb_calls; /* max_rows: the largest rows_bound() of a named buffer when its call was queued */
  bool begun, failed, tab_pending;
} EdgeStore;

/* What vksift_ext_selectTrackObservations keeps (vksift_observations.c), sized like the tracks it reads: at most cap_bufs * max_nb_sift_per_buffer
 * observations of half as many tracks. Allocated by the first selection. `valid`: cleared wherever tracks.valid is, and by a new build. */
typedef struct
{
  uint32_t *d_offsets, *d_track_ids; /* CSR offsets (tracks + 1 words) and the selected tracks' numbers */
  uint8_t *d_obs;                    /* the vksift_ext_Observation records */
  uint32_t *d_stats, *h_stats;       /* the four words of vksift_ext_ObservationStats, posted */
  uint32_t *d_scratch;               /* coordinates, sort lists, digit table, map (vksift_hip_observations_scratch_u32) */
  size_t scratch_u32;
  uint32_t *h_tab;                   /* mapped pinned memory read by the launches: cap_bufs section tables (buffer_layouts), then one layout word per rank */
  bool valid, tab_pending;
} ObservationResults;

/* What vksift_ext_triangulateTracks keeps (vksift_triangulate.c): one point per selected track, at most half as many as there are nodes. Allocated by the
 * first triangulation. `valid`: cleared wherever obs.valid is, and by a new selection. */
typedef struct
{
  uint8_t *d_points;           /* the vksift_ext_Point records */
  uint32_t *d_stats, *h_stats; /* the four words of vksift_ext_PointStats, posted */
  float *h_cameras, *d_cameras; /* 12 floats per SIFT buffer: filled in pinned memory by the call, copied to the device in front of the launches */
  bool valid, cam_pending;
} TriangulateResults;

/* What vksift_ext_indexObservationsByView keeps (vksift_cameras.c): the observation table by view, an entry per observation at most and an offset per
 * SIFT buffer. Allocated by the first index. `valid`: cleared wherever obs.valid is. */
typedef struct
{
  uint32_t *d_offsets;         /* sift_buffer_count + 1 words, indexed by gpu_buffer_id */
  uint8_t *d_obs;              /* the vksift_ext_ViewObservation records */
  uint32_t *d_stats, *h_stats; /* the four words of vksift_ext_ViewStats, posted */
  uint32_t *d_scratch;         /* sort lists, the observations' points, digit table (vksift_hip_views_scratch_u32) */
  size_t scratch_u32;
  bool valid;
} ViewResults;

/* What vksift_ext_refineCameras keeps (vksift_cameras.c): one record per SIFT buffer. Allocated by the first refinement. `valid`: cleared wherever
 * tri.valid is, and by a new triangulation (the records refer to its points and cameras). */
typedef struct
{
  uint8_t *d_refined;          /* the vksift_ext_RefinedCamera records */
  uint32_t *d_stats, *h_stats; /* the four words of vksift_ext_CameraStats, posted */
  bool valid;
} CameraResults;

typedef struct
{
  vksift_hip_event ev_t[8];  /* instance stream: start, upload end, pyramid end, extrema end, orientation end, descriptor end, call end */
  vksift_hip_event ev_pt[3]; /* start / end of octave 0's scale-space construction on its own stream (overlapping detections); [2]: end of the last octave's */
  vksift_hip_event ev_scan;  /* octave 0's streaming extrema scan (the kernel that forms the DoG values) has run */
  bool valid, accounted, overlap;
  uint32_t blur_launches, blur_launches_all;
  uint64_t alg_bytes, scan_bytes;
} ProfSet;

/* Fields grouped by who uses them. Every pointer to device (d_), pinned (h_) or heap memory and every event and stream of the struct is
 * listed once in the tables of vksift_mem.c (blocks[], handles[]), which creation, growth and release walk. */
struct vksift_Instance_T
{
  vksift_Config cfg;
  void (*error_cb)(vksift_Result);
  int device;
  uint32_t S;
  bool fp16;               /* VKSIFT_PYRAMID_PRECISION_FLOAT16: the scale-space holds IEEE binary16 texels (2 bytes), arithmetic stays fp32 */
  uint32_t max_image_size; /* rounded up to a square, sift_memory.c:644-647 */
  uint32_t max_octaves;
  uint32_t batch_cap;      /* capacity the instance was created with: match slots, and the bound of the vksift_ext_*Batch entries */
  uint32_t det_cap;        /* images one detection launch sequence can take (>= batch_cap): input staging, scale-space, extraction scratch.
                            * Grows when a caller of the plain API turns out to batch (deferred submission, below) */
  /* blur taps */
  float taps[(VKSIFT_MAX_SCALES + 3) * VKSIFT_MAX_TAPS];
  uint32_t ntaps[VKSIFT_MAX_SCALES + 3];

  /* ---- deferred submission of vksift_detectFeatures (vksift_defer.c: defer_detect). The reference's caller hands over ONE image per call
   * (vulkansift.c:315-344); a caller that issues several such calls in a row, into consecutive SIFT buffers, before it asks for
   * anything gets them launched as ONE batched detection: the call stages its image in the pinned input block and returns, and the
   * batch is launched by the first call that needs a result (every other entry point: defer_sync) or when it is full. The first
   * detection after an accessor is launched at once unless the caller is known to batch (batch_mode), so detect + read keeps its path. */
  bool defer_enabled;      /* VKSIFT_DEFER (default 1) and sift_buffer_count >= 2 */
  uint32_t defer_max;      /* VKSIFT_DEFER_MAX (default 128): a deferred batch is launched when it holds this many images (or det_cap) */
  uint32_t defer_chunk;    /* VKSIFT_DEFER_CHUNK (default 16; 0: off): ... or this many while the GPU has no detection to work on */
  uint32_t pend_n, pend_first, pend_w, pend_h; /* staged images: SIFT buffers [pend_first, pend_first + pend_n) */
  uint32_t epoch_detects;  /* vksift_detectFeatures calls since the last call of any other entry point */
  bool batch_mode;         /* the last such run held at least two: the next one is deferred from its first call on */
  bool defer_grow;         /* the last deferred batch filled det_cap: double it before the next one is staged */
  uint64_t defer_batches, defer_images; /* statistics (vksift_ext_getDeferredStats) */

  /* ---- how a detection is scheduled (read_switches, vksift_instance.c) */
  bool pyr_pingpong;       /* overlap mode: the scale-space of a detection is built on its own stream, beside what is queued behind the previous detection's descriptors */
  uint32_t overlap_min_count; /* ... for detections of at least this many images (1; 8 on an instance whose capacity grew by deferred submission) */
  bool overlap_forced;     /* VKSIFT_PYR_PINGPONG was given: the mode is the caller's */
  uint32_t pyr_nbuf;       /* scale-space buffers of the instance: 1, or 2 with VKSIFT_PYR_PINGPONG=2 (the next scale-space may then start before the previous detection's readers are done) */
  /* small detections (one image): the scales behind scale S of an octave are off the path to the next octave; they run on the
   * (otherwise idle) scale-space stream beside the octaves below — forked per octave, joined in front of the keypoint stages */
  int fork_streams;              /* branch streams of a forked detection: 1 (two measured no faster in stream order, slower in a graph) */
  bool fork_scales; /* VKSIFT_FORK_SCALES (default 1) */
  uint64_t fork_max_pixels; /* ... for detections of at most this many input pixels (16 Mpx) */
  uint32_t lds_chain_max; /* largest plane (texels) an octave of the chain may have: VKSIFT_LDS_CHAIN_MAX, at most 19200 (the LDS) */
  bool lds_chain_refuse; /* VKSIFT_LDS_CHAIN=refuse: test hook, the chain launch declines and the per-scale launches take over */
  bool lds_chain; /* VKSIFT_LDS_CHAIN (default 1): the trailing octaves that fit the LDS are built by one launch (vksift_hip_octave_chain) */
  bool alt_order; /* always on: launches of a blur chain alternate their dispatch direction (vksift_hip_Plane::reverse) */
  /* hipGraph replay of the detection launch sequence (latency of small workloads is launch bound) */
  bool use_graphs;
  uint64_t graph_max_pixels; /* detections of at most this many input pixels (batch total) are replayed from a graph */
  DetectGraph graphs[VKSIFT_GRAPH_CACHE];
  uint64_t graph_stamp;
  uint32_t graph_miss_run; /* consecutive cache misses: a caller that never repeats a key gets no replays, only capture costs */

  /* ---- current scale-space */
  uint32_t cur_w, cur_h, cur_batch;
  uint32_t shown_img;      /* image of the last launch the scale-space accessors show: the last one of a batch launched from staged
                            * vksift_detectFeatures calls (the reference shows the last image detected), image 0 otherwise */
  PyrLayout lay;
  float *d_pyr;            /* pyramid storage of the current detection (= d_pyr_buf[pyr_cur]); texel offsets scale with pyr_texel_bytes() */
  int pyr_cur;
  bool pyr_free_valid[2];

  /* ---- detection scratch: re-allocated by resize_detect_scratch when the per-image strides or the capacity grow */
  float *d_pyr_buf[2];     /* the scale-space buffer(s): ONE by default (the overlap gate makes a second unnecessary), two with VKSIFT_PYR_PINGPONG=2 */
  uint32_t place_n;        /* candidate ranges timed by place_pyramid_buffers (0: plain allocation), their rates, the chosen ones */
  float place_gbps[8];
  uint32_t place_chosen[2];
  uint64_t pyr_img_stride; /* floats reserved per image */
  uint64_t *d_seg_mask;    /* per stride */
  uint32_t *d_seg_off;
  uint64_t seg_cap; /* elements reserved per image */
  uint32_t *d_cand_xy, *d_cand_flag;
  uint64_t cand_cap; /* candidates reserved per image */
  uint8_t *d_input, *h_input; /* per capacity */
  uint32_t *d_cand_n;
  float *d_ori_ang;
  uint32_t *d_ori_cnt;
  uint64_t ori_cap; /* keypoints reserved per image */

  /* ---- the SIFT buffers (fixed at creation) */
  uint8_t *d_feats;
  uint64_t buf_stride; /* bytes */
  uint32_t *d_found, *h_found;
  BufferInfo *bufs;
  float *d_desc_fp;
  uint32_t desc_fp_len;

  /* ---- matcher */
  uint8_t *d_matches, *h_matches; /* (h_matches: pinned, the packed download of a batched matching, allocated by it) */
  uint32_t *d_redo;        /* per match slot: row flags for the exact scalar replay (k_match_redo) */
  uint32_t *d_match_n, *h_match_n; /* per match slot: {N_A, N_B, spare, spare} of the last matching pipeline */
  uint64_t desc_slot_stride, match_slot_stride; /* bytes */
  uint64_t redo_slot_stride;                    /* u32 elements */
  uint32_t match_slots_used; /* (the plain matching's records keep a download path of their own, md_*: not a PairResults) */
  /* per SIFT buffer: the matcher's view of it (dense descriptor rows in download order, shifted norms, row count), filled by a
   * device-side gather when the buffer is first matched after a detection / upload; desc, norm and the partial lists: first matching */
  uint8_t *d_cache_desc;
  uint32_t *d_cache_norm, *d_cache_n;
  uint64_t cache_norm_stride; /* u32 elements */
  bool *cache_valid;
  bool *cache_queued;      /* scratch of refresh_match_cache: the buffer is already in the current gather pass */
  uint32_t *d_match_partial; /* partial top-2 lists of the stream-decomposed single-pair matcher (NULL when max_nb <= VKSIFT_HIP_MATCH_SMALL_NA) */
  bool match_pending;
  bool *match_busy; /* per SIFT buffer: read by the matching pipeline in flight (all pairs of a batched call) */
  uint32_t curr_nb_matches;
  /* packed download of the records of a batched matching (h_matches) */
  size_t md_cap, md_pitch;
  bool md_valid;
  bool md_asked, md_direct;  /* (asked once per matching) the caller's destination of this matching's records is page-locked: per-pair DMA, no packed copy */
  uint32_t md_hits;

  /* ---- the stages behind a filtered matching (vksift_pairs.c): what each keeps per pair, and its scratch; everything allocated on first use */
  PairResults res[PR_COUNT];
  MatchScratch rev;         /* vksift_ext_matchFeaturesFiltered: scratch of the reverse (B->A) matching */
  /* geometric verification (vksift_ext_verifyHomography / vksift_ext_verifyFundamental, vksift_verify.c). Each model keeps records and masks of its
   * own, so that both can be read after one matching; the refits (vksift_refine.c) read d_corr and their model's verified records and masks */
  uint32_t *filt_ids;       /* 2 * batch_cap: buffers A then buffers B of the last vksift_ext_matchFeaturesFiltered */
  float *d_corr;            /* per slot: res[PR_FILTERED].stride bytes of {xa, ya, xb, yb} */
  uint32_t *d_vscratch;
  size_t vscratch_u32;
  uint32_t *h_vtab;         /* mapped pinned memory read by the gather launch: a pair table (pair_tables) */
  bool vtab_pending;
  /* guided matching (vksift_ext_matchFeaturesGuided, vksift_guided.c) */
  float *d_gxy;             /* per slot: 2 * gxy_side_stride float2, the coordinates of A's rows, then of B's */
  uint64_t gxy_side_stride; /* float2 elements */
  uint32_t *d_gkeys;        /* the sweeps' top-2 keys (vksift_hip_guided_scratch_u32) */
  size_t gkeys_u32;
  uint32_t *h_gtab;         /* mapped pinned memory read by the launches: a pair table (pair_tables), then 9 floats per slot of supplied models and
                             * a word 1 per slot */
  bool gtab_pending;
  /* feature tracks over the pair list (vksift_ext_buildTracks, vksift_tracks.c) */
  TrackResults tracks;
  /* the edge store of tracks across matching calls (vksift_ext_beginTrackAccumulation, vksift_track_edges.c) */
  EdgeStore edges;
  /* the observation table of selected tracks (vksift_ext_selectTrackObservations, vksift_observations.c) */
  ObservationResults obs;
  /* the points of the selected tracks under caller-supplied cameras (vksift_ext_triangulateTracks, vksift_triangulate.c) */
  TriangulateResults tri;
  /* the observation table by view, and the cameras refined on the points (vksift_ext_indexObservationsByView, vksift_ext_refineCameras, vksift_cameras.c) */
  ViewResults views;
  CameraResults cams;

  /* ---- caller-supplied keypoints (vksift_describe.c); everything allocated by the first describe call */
  uint8_t *d_kps, *h_kps;        /* one call's keypoint offsets (count + 1 words, padded to 256 bytes) and, behind them, its keypoints: pinned staging and the device copy */
  size_t kps_cap;                /* bytes of each (grows with the largest call) */
  uint32_t *d_placed, *h_placed; /* per SIFT buffer: the records its last placement stored, before orientation copies */
  uint64_t *placed_seq;          /* per SIFT buffer: the describe call whose count h_placed holds (0: none) */

  /* ---- download staging. Batched download: the first vksift_downloadFeatures() after a detection of VKSIFT_DL_BATCH_MIN images and more
   * packs the features of ALL its buffers on the device and fetches them with one copy into pinned memory; the downloads of the
   * other buffers are host copies out of it (one copy per section and buffer costs 80 us per buffer otherwise) */
  uint8_t *d_dl, *h_dl; /* the staging pair (mem_fit_staging) */
  size_t dl_cap;       /* bytes of each */
  uint32_t *dl_row;    /* sift_buffer_count + 1 row offsets of the cached buffers */
  uint32_t dl_first, dl_count;
  bool dl_valid;
  bool dl_direct;            /* the packed copy of the current detection is fetched by DMA into page-locked destinations: nothing went to h_dl */
  size_t dl_chunk_end[VKSIFT_DL_CHUNKS];
  uint32_t dl_chunks, dl_chunks_done;
  uint64_t dl_seq;      /* the detection the packed copy belongs to */
  uint64_t dl_hits_seq; /* the detection dl_hits counts for */
  uint32_t dl_hits; /* vksift_downloadFeatures calls on buffers of that detection, before its packed copy exists */

  /* ---- feature posting: a single-image detection ends with the pack kernel storing the dense records of its buffer straight into
   * mapped pinned memory (slot = buffer index & 1), so that vksift_getFeaturesNumber + vksift_downloadFeatures cost ONE host wait
   * and a host copy — instead of wait, pack launch, device-to-host copy, second wait (~60 us of a 0.45 ms detection).
   * Costs bus time when nobody downloads: switched off after VKSIFT_POST_IDLE posted detections in a row that were never
   * fetched, on again by the next download of a single detection. VKSIFT_POST_FEATURES=0 disables. */
  uint8_t *h_post[2];     /* allocated by the first detection that posts */
  size_t post_cap;        /* bytes of each */
  uint64_t post_seq[2];   /* detection whose records the slot holds (0: none) */
  uint32_t post_buf[2];
  bool post_fetched[2];   /* the slot's records were downloaded at least once */
  bool post_enabled, post_on;
  uint32_t post_idle;

  /* ---- streams and events (ProfSet and DetectSlot hold more events) */
  vksift_hip_stream stream;
  vksift_hip_stream pyr_stream; /* scale-space construction when detections overlap (two pyramid buffers) */
  vksift_hip_stream up_stream;  /* host-to-device copies of the input images */
  vksift_hip_stream dl_stream;  /* result downloads: the accessors have waited for the pipeline that produced what they read; their copies must
                                 * not queue behind a LATER detection already on the instance stream (a caller that pipelines) */
  vksift_hip_stream side_stream; /* second branch stream of a forked detection (the first is pyr_stream) */
  vksift_hip_event ev_pyr_done;
  vksift_hip_event ev_pyr_free[2]; /* last reader of pyramid buffer i has finished */
  vksift_hip_event ev_desc_start;  /* the previous detection's descriptor stage has been issued up to here: the next scale-space may start */
  vksift_hip_event ev_input_free;  /* the last reader of d_input (seed pass of the most recent detection) has run */
  vksift_hip_event ev_fork[VKSIFT_MAX_OCTAVES], ev_join[2]; /* forked detections */
  vksift_hip_event ev_staging;      /* host image staging buffer consumed by the H2D copy */
  vksift_hip_event ev_up[VKSIFT_UP_GROUPS]; /* group g of a batch has arrived in d_input */
  vksift_hip_event ev_match;
  StageTimer timer[T_COUNT];        /* profiling: the stages' intervals. The matching's events are created with the instance, the others by their first timed run */
  vksift_hip_event dl_ev[VKSIFT_DL_CHUNKS]; /* the packed copy arrives in pieces (created by the first one) */
  vksift_hip_event ev_vtab; /* the last gather launch has read h_vtab (created by the first verification) */
  vksift_hip_event ev_gtab; /* the last guided matching has read h_gtab (created by the first guided matching) */
  vksift_hip_event ev_ttab; /* the last track build has copied tracks.h_tab (created by the first build) */
  vksift_hip_event ev_etab; /* the last accumulate has copied edges.h_tab (created by the first accumulation) */
  vksift_hip_event ev_otab; /* the last observation launches have read obs.h_tab (created by the first selection) */
  vksift_hip_event ev_ctab; /* the last triangulation has copied tri.h_cameras (created by the first triangulation) */
  vksift_hip_event ev_kps;  /* the last describe call's copy has read h_kps (created by the first describe call) */
  bool desc_start_valid, input_free_valid, staging_pending, kps_pending;
  DetectSlot det_ring[VKSIFT_DETECT_RING];
  uint64_t det_seq, det_done; /* last detection issued / highest one known to have completed */

  /* ---- profiling */
  bool profiling;
  ProfSet prof[2]; /* two event sets: the host may enqueue one detection ahead of the one being timed */
  int prof_cur;
  double acc_ms[8]; /* upload, pyramid (octave 0), extrema stage, orientation, descriptor, total, extrema scan kernel alone, pyramid (all octaves) */
  uint32_t acc_calls;
  uint64_t acc_blur_launches, acc_blur_launches_all, acc_alg_bytes, acc_scan_bytes;
  uint32_t last_blur_launches, last_blur_launches_all;
  uint64_t last_alg_bytes, last_scan_bytes;
  bool device_input_last;
};


#define HIP_CHECK(expr, what)                                                      \
  do                                                                               \
  {                                                                                \
    int _e = (expr);                                                               \
    if (_e != 0)                                                                   \
    {                                                                              \
      logError(LOG_TAG, "%s failed: %s", what, vksift_hip_error_string(_e));       \
      goto gpu_error;                                                              \
    }                                                                              \
  } while (0)

static inline size_t pyr_texel_bytes(const struct vksift_Instance_T *inst) { return inst->fp16 ? 2u : 4u; }
/* address of texel `off` (texels from the start of the pyramid buffer) */
static inline float *pyr_at(const struct vksift_Instance_T *inst, uint64_t off) { return (float *)((uint8_t *)inst->d_pyr + off * pyr_texel_bytes(inst)); }

static inline bool counts_valid(const struct vksift_Instance_T *inst, uint32_t buf) { return inst->bufs[buf].seq <= inst->det_done; }

/* vksift_api.c */
extern VKSIFT_INTERNAL bool vksift_g_loaded;
VKSIFT_INTERNAL bool config_is_valid(const vksift_Config *c);
VKSIFT_INTERNAL void default_error_callback(vksift_Result err);
VKSIFT_INTERNAL bool buffer_idx_valid(vksift_Instance inst, uint32_t idx);
VKSIFT_INTERNAL bool resolution_valid(vksift_Instance inst, uint32_t w, uint32_t h);

/* vksift_mem.c */
typedef enum { MEM_DEVICE, MEM_PINNED, MEM_HEAP } MemKind;
VKSIFT_INTERNAL void compute_layout(vksift_Instance inst, uint32_t w, uint32_t h, PyrLayout *L);
/* field: address of a pointer of the instance. Allocates `bytes` of that kind unless the block exists (a group that ran out of memory
 * half-way is retried without leaking); false: out of memory. mem_release frees it and clears the pointer. */
VKSIFT_INTERNAL bool mem_ensure(void *field, size_t bytes, MemKind kind);
VKSIFT_INTERNAL void mem_release(void *field, MemKind kind);
/* the staging pair d_dl / h_dl holds `bytes` (re-allocated with 25 % on top when it does not, or when may_shrink and it is far too
 * large); false: out of memory, both pointers NULL and dl_cap 0 */
VKSIFT_INTERNAL bool mem_fit_staging(vksift_Instance inst, size_t bytes, bool may_shrink);
VKSIFT_INTERNAL bool mem_create(vksift_Instance inst, const PyrLayout *L);
VKSIFT_INTERNAL int mem_resize_scratch(vksift_Instance inst, const PyrLayout *L, uint32_t new_cap);
VKSIFT_INTERNAL void mem_destroy(vksift_Instance inst);

/* vksift_instance.c */
VKSIFT_INTERNAL void set_buffer_sections(vksift_Instance inst, uint32_t buf, uint32_t n_oct, uint32_t w, uint32_t h);
VKSIFT_INTERNAL void mark_detect_done(vksift_Instance inst);
VKSIFT_INTERNAL bool detect_running(vksift_Instance inst);
VKSIFT_INTERNAL int wait_detect_seq(vksift_Instance inst, uint64_t seq);
VKSIFT_INTERNAL int wait_detect_passed(vksift_Instance inst, uint64_t seq);
/* buffers [first, first + count) are rewritten in place by what the caller queues next (vksift_strongest.c, vksift_rootsift.c): they take the next
 * sequence number and a ring slot; the caller records the slot's event behind its launches */
VKSIFT_INTERNAL void take_sequence(vksift_Instance inst, uint32_t first, uint32_t count);
VKSIFT_INTERNAL bool match_running(vksift_Instance inst);
VKSIFT_INTERNAL int wait_all(vksift_Instance inst);
VKSIFT_INTERNAL int grow_image_scratch(vksift_Instance inst, const PyrLayout *L);
VKSIFT_INTERNAL int resize_detect_scratch(vksift_Instance inst, const PyrLayout *L, uint32_t new_cap);
VKSIFT_INTERNAL void drop_detect_graphs(vksift_Instance inst);

/* vksift_stage.c: images [i0, i1) -> dst (the pinned staging buffer), by a small pool of copy threads */
VKSIFT_INTERNAL void stage_images(uint8_t *dst, const uint8_t *const *images, uint32_t i0, uint32_t i1, size_t img_bytes);

/* vksift_detect.c */
VKSIFT_INTERNAL bool detect_args_valid(vksift_Instance inst, uint32_t count, uint32_t w, uint32_t h, uint32_t first_buf, bool report);
VKSIFT_INTERNAL void detect_impl(vksift_Instance inst, const uint8_t *const *images, const uint8_t *d_images, bool prestaged, uint32_t count, uint32_t w,
                                 uint32_t h, uint32_t first_buf, const char *fn);
VKSIFT_INTERNAL void account_set(vksift_Instance inst, ProfSet *ps);
VKSIFT_INTERNAL void account_timings(vksift_Instance inst);

/* vksift_defer.c */
VKSIFT_INTERNAL void flush_deferred(vksift_Instance inst);
/* Every entry point but vksift_detectFeatures starts with this: what was deferred is launched, and the run of detect calls ends */
static inline void defer_sync(vksift_Instance inst)
{
  if (inst->pend_n)
    flush_deferred(inst);
  if (inst->epoch_detects)
  {
    inst->batch_mode = inst->epoch_detects >= 2u;
    inst->epoch_detects = 0;
  }
}

/* vksift_buffers.c */
VKSIFT_INTERNAL void wait_for_buffer(vksift_Instance inst, uint32_t buf);
VKSIFT_INTERNAL uint32_t buffer_counts(vksift_Instance inst, uint32_t buf, uint32_t *cnt, bool log_lost);

/* vksift_match.c */
/* the matcher's cache blocks as the launches over sectioned buffers take them; all NULL until the first matching has made them */
typedef struct
{
  uint8_t *desc;
  uint32_t *norm, *n;
} CacheBlocks;
static inline CacheBlocks cache_blocks(const struct vksift_Instance_T *inst)
{
  const bool made = inst->d_cache_desc && inst->d_cache_norm;
  return (CacheBlocks){made ? inst->d_cache_desc : NULL, made ? inst->d_cache_norm : NULL, made ? inst->d_cache_n : NULL};
}
VKSIFT_INTERNAL MatchScratch fwd_scratch(vksift_Instance inst);
VKSIFT_INTERNAL int refresh_match_cache(vksift_Instance inst, const uint32_t *ids, uint32_t count);
VKSIFT_INTERNAL uint32_t rows_bound(vksift_Instance inst, uint32_t id);
VKSIFT_INTERNAL void wait_match(vksift_Instance inst);
/* What every launch sequence queued on the matching's contract ends with (the matching itself, the verification, the guided matching): the
 * accessors wait for ev_match, both buffers of every pair stay busy until it has passed. Returns the event record's error code. */
VKSIFT_INTERNAL int match_follow(vksift_Instance inst, const uint32_t *ids_a, const uint32_t *ids_b, uint32_t count);

/* The pair table of the launches that resolve download-order rows on the device (vksift_hip_gather_correspondences, vksift_hip_gather_xy;
 * h_vtab, h_gtab): {buffer A, buffer B, layout A, layout B} per slot of batch_cap, then the section tables the layout words name (hip/records.h;
 * at most one per buffer). pair_tables fills it for the `count` pairs of the last filtered matching; max_rows, unless NULL, receives the
 * largest rows_bound() of their buffers, at most max_nb_sift_per_buffer. */
#define PAIR_SLOT_WORDS 4u
static inline uint32_t *pair_layouts(const struct vksift_Instance_T *inst, uint32_t *tab) { return tab + (size_t)PAIR_SLOT_WORDS * inst->batch_cap; }
static inline size_t pair_table_words(const struct vksift_Instance_T *inst) { return ((size_t)PAIR_SLOT_WORDS + (size_t)VKSIFT_LAYOUT_WORDS * 2u) * inst->batch_cap; }
VKSIFT_INTERNAL void pair_tables(vksift_Instance inst, uint32_t *tab, uint32_t count, uint32_t *max_rows);
/* the layout words of n buffers, whichever pair list they were in: words[i] names the section table of ids[i] among those appended to `layouts` (at most n
 * tables of VKSIFT_LAYOUT_WORDS), as the layout words of a pair table do */
VKSIFT_INTERNAL void buffer_layouts(vksift_Instance inst, const uint32_t *ids, uint32_t n, uint32_t *words, uint32_t *layouts);

/* vksift_tracks.c */
/* the record set (and the set whose masks and valid words select among its records, or NULL) a VKSIFT_EXT_TRACKS_* source takes its edges from; false: no
 * filtered matching, an unknown source, or a source whose stage has not run for the present matching */
VKSIFT_INTERNAL bool track_source(vksift_Instance inst, uint32_t source, const PairResults **rec, const PairResults **sel);
/* the tracks' storage for tracks.cap_bufs buffers (allocated by the first build of either kind); false: out of memory */
VKSIFT_INTERNAL bool track_storage_ensure(vksift_Instance inst);
/* what both builds fill for one pair list: rank_of (per SIFT buffer; VKSIFT_EXT_NO_TRACK outside the list), {rank A, rank B} per slot, {gpu_buffer_id, word of
 * d_match_n} per rank and, unless NULL, ids and count_word per rank. Returns the number of buffers; *max_rows: the largest rows_bound() among them, 1 at least */
VKSIFT_INTERNAL uint32_t pair_list_ranks(vksift_Instance inst, uint32_t count, uint32_t *rank_of, uint32_t *slot_tab, uint32_t *buf_tab, uint32_t *ids, uint32_t *count_word,
                                         uint32_t *max_rows);
/* a build of either kind replaces the tracks: they and everything computed from them are not served any more */
static inline void tracks_invalidate(vksift_Instance inst) { inst->tracks.valid = inst->obs.valid = inst->tri.valid = inst->views.valid = inst->cams.valid = false; }


/* vksift_pairs.c */
/* a stage's time getter: the interval of its last run in ms, -1 unless profiling is on and the stage has run since it was switched on */
VKSIFT_INTERNAL float timer_read(vksift_Instance inst, uint32_t timer);
VKSIFT_INTERNAL void timers_reset(vksift_Instance inst);
/* The frame around the launches of a stage. stage_begin starts the timer (when profiling; its events are created by the first timed run) and opens
 * the profiler range; stage_end closes the range, stops the timer and, given the pairs, ends the sequence the way every one queued on the matching's
 * contract does (match_follow, whose error code it returns). stage_abort, for the error exit, closes the range if it is open and says whether it was. */
typedef struct
{
  StageTimer *timer;
  bool open;
  bool begun; /* stage_begin has succeeded: launches of the call may be queued */
} StageFrame;
VKSIFT_INTERNAL int stage_begin(vksift_Instance inst, StageFrame *f, uint32_t timer, const char *range);
VKSIFT_INTERNAL int stage_end(vksift_Instance inst, StageFrame *f, const uint32_t *ids_a, const uint32_t *ids_b, uint32_t count);
VKSIFT_INTERNAL bool stage_abort(StageFrame *f);
/* The error exit of a stage queued on the matching's contract. Whatever part of the call was queued still reads the pairs' buffers (and posts into the
 * words the accessors read): the range is closed and, once stage_begin has succeeded, the sequence ends the way a complete one does (match_follow) — or,
 * if that record fails too, behind a drained stream — so that vksift_isBufferAvailable and the accessors wait for it. */
VKSIFT_INTERNAL void stage_fail(vksift_Instance inst, StageFrame *f, const uint32_t *ids_a, const uint32_t *ids_b, uint32_t count);

/* vksift_instance.c, behind take_sequence: what the calls that rewrite a range of SIFT buffers in place share (vksift_strongest.c, vksift_rootsift.c). They are queued like a
 * detection: between the two halves the caller opens its stage, takes the sequence number (take_sequence) and makes one launch per layout run. */
static inline bool inplace_range_valid(const struct vksift_Instance_T *inst, uint32_t first, uint32_t count)
{
  return count != 0 && count <= VKSIFT_HIP_GATHER_SLOTS && first < inst->cfg.sift_buffer_count && count <= inst->cfg.sift_buffer_count - first;
}
/* waits for a direct packed download that may still read the records, polls the detections in flight (counts_valid() and rows_bound() are up to
 * date) and fills ids[0 .. count) with first + i. Returns the wait's error code, ids filled or not. */
VKSIFT_INTERNAL int inplace_begin(vksift_Instance inst, uint32_t first, uint32_t count, uint32_t *ids);
/* closes the stage; the call ends on the event of its detection-ring slot, not on pairs. Returns the event record's error code. */
VKSIFT_INTERNAL int inplace_end(vksift_Instance inst, StageFrame *f);
/* the error exit: the slot's event behind whatever part of the call was queued, `msg` logged, VKSIFT_VULKAN_ERROR reported */
VKSIFT_INTERNAL void inplace_fail(vksift_Instance inst, StageFrame *f, const char *msg);
/* storage of batch_cap pairs for set `which` (PR_*) with this shape; false: out of memory (retried by the next call, nothing leaked) */
VKSIFT_INTERNAL bool pair_results_ensure(vksift_Instance inst, uint32_t which, uint32_t words, uint64_t stride, uint32_t elem, uint32_t counted_by);
/* a new matching: no set has results any more */
VKSIFT_INTERNAL void pair_results_invalidate(vksift_Instance inst);
/* The accessors. Both wait for the pipeline in flight (wait_match), then refuse a pair the set has no results for (and !out_ok: the caller's output
 * pointer is NULL) with a log line under the public entry's name `fn` and VKSIFT_INVALID_INPUT_ERROR. pair_words: the pair's posted words, NULL when
 * refused. pair_download: the pair's payload to dst through dl_stream (nothing when it is empty); `what` and `noun` word the failure's log lines. */
VKSIFT_INTERNAL const uint32_t *pair_words(vksift_Instance inst, uint32_t which, uint32_t pair, bool out_ok, const char *fn);
VKSIFT_INTERNAL void pair_download(vksift_Instance inst, uint32_t which, uint32_t pair, void *dst, const char *fn, const char *what, const char *noun);

#endif
