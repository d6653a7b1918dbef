/*
 * vksift_ext.h — additive extensions to the vksift_* API for the MI355X build.
 *
 * Nothing here exists in the reference; none of it changes the layout or behaviour of the reference
 * API (include/vulkansift/vulkansift.h). The extensions expose what a 288 GB / 8 TB/s device makes
 * worthwhile: batched detection (the reference handles one image at a time per instance,
 * vulkansift.c:326-327), device-resident inputs/outputs for multi-GPU pipelines, and stage timings
 * taken with HIP events on the instance's own stream.
 */
#ifndef VKSIFT_EXT_H
#define VKSIFT_EXT_H

#include "vulkansift/vulkansift.h"

#ifdef __cplusplus
extern "C"
{
#endif

  /* Like vksift_createInstance, but reserves `batch_capacity` pyramids so that up to that many
   * same-sized images can be processed by one vksift_ext_detectFeaturesBatch call.
   * config->sift_buffer_count must be >= batch_capacity. */
  VKSIFT_EXPORT vksift_Result vksift_ext_createInstanceBatched(vksift_Instance *instance_ptr, const vksift_Config *config, uint32_t batch_capacity);

  /* Detect on `count` images of identical resolution; image i fills SIFT buffer first_gpu_buffer_id+i.
   * Same asynchronous contract and error behaviour as vksift_detectFeatures. */
  VKSIFT_EXPORT void vksift_ext_detectFeaturesBatch(vksift_Instance instance, const uint8_t *const *images, uint32_t count, uint32_t image_width,
                                                    uint32_t image_height, uint32_t first_gpu_buffer_id);
  /* Same, images already in device memory (contiguous, image i at d_images + i*width*height). */
  VKSIFT_EXPORT void vksift_ext_detectFeaturesBatchDevice(vksift_Instance instance, const uint8_t *d_images, uint32_t count, uint32_t image_width,
                                                          uint32_t image_height, uint32_t first_gpu_buffer_id);

  /* 2-NN matching of `count` buffer pairs (A[i], B[i]) in one launch sequence; count <= batch capacity.
   * Same asynchronous contract and error behaviour as vksift_matchFeatures; pair 0 is also what
   * vksift_getMatchesNumber / vksift_downloadMatches return.
   * A call that fails with VKSIFT_VULKAN_ERROR (here, and in every stage queued behind a matching: filtered matching, verification, refit,
   * guided matching, tracks): a result whose device storage a launch of the failed call had begun to overwrite is refused by all its
   * accessors (VKSIFT_INVALID_INPUT_ERROR), together with what was computed from it — after a failed matching every per-pair result and the
   * tracks, after a failed verification its model's records, masks and refit —, until a later call has succeeded; every other result stays
   * served and unchanged; the buffers of the pairs stay busy (vksift_isBufferAvailable) until what was queued has run.
   * vksift_downloadMatches and vksift_ext_downloadMatchesBatch(0) keep the reference's contract, which knows no refusal: after a failed
   * matching they return as many records as vksift_getMatchesNumber counts, of unspecified content. */
  VKSIFT_EXPORT void vksift_ext_matchFeaturesBatch(vksift_Instance instance, uint32_t count, const uint32_t *gpu_buffer_ids_A,
                                                   const uint32_t *gpu_buffer_ids_B);
  VKSIFT_EXPORT uint32_t vksift_ext_getMatchesNumberBatch(vksift_Instance instance, uint32_t pair);
  VKSIFT_EXPORT void vksift_ext_downloadMatchesBatch(vksift_Instance instance, uint32_t pair, vksift_Match_2NN *matches);

  /* ---- GPU-side match filtering ------------------------------------------------------------------
   * What callers of the reference do on the CPU after vksift_downloadMatches (src/examples/test_sift_match.cpp:90-107,
   * src/perf/perf_common.cpp:123-169): match A->B and, with cross_check, B->A; keep a match iff it is mutual and passes
   * Lowe's ratio test d1/d2 < ratio (in both directions when cross-checking). Only the survivors (16 B each, increasing
   * idx_a) leave the GPU. Asynchronous like vksift_matchFeatures; the forward 2-NN records stay available through
   * vksift_getMatchesNumber / vksift_downloadMatches (pair 0) and the ...Batch accessors. count <= batch capacity. */
  typedef struct
  {
    uint32_t idx_a, idx_b;
    float dist_a_b1, dist_a_b2;
  } vksift_ext_FilteredMatch;
  VKSIFT_EXPORT void vksift_ext_matchFeaturesFiltered(vksift_Instance instance, uint32_t count, const uint32_t *gpu_buffer_ids_A,
                                                      const uint32_t *gpu_buffer_ids_B, float ratio, bool cross_check);
  VKSIFT_EXPORT uint32_t vksift_ext_getFilteredMatchesNumber(vksift_Instance instance, uint32_t pair);
  VKSIFT_EXPORT void vksift_ext_downloadFilteredMatches(vksift_Instance instance, uint32_t pair, vksift_ext_FilteredMatch *matches);

  /* ---- GPU-side geometric verification --------------------------------------------------------------------------------
   * What callers do next with filtered matches: a RANSAC homography per pair, here for every pair of the last vksift_ext_matchFeaturesFiltered call in
   * three launches, without downloading matches or features. nb_hypotheses (1 .. 65536) four-point samples per pair, drawn from a counter-based generator
   * keyed by (seed, pair, hypothesis); a match is an inlier when the forward transfer error of its A keypoint is below threshold_px (and it is not mapped
   * behind the plane); the model with the most inliers wins, ties to the lowest hypothesis. Deterministic: the same inputs give the same bytes on every run
   * (tests/np_verify.py restates the estimator bit for bit). No refit on the inliers in this call (H is the four-point model of the winning sample):
   * vksift_ext_refineHomography (below) refits it on the GPU; the mask is also what a caller's own least-squares refinement needs.
   * Asynchronous like the matching entry points: queued behind the matching, the pairs' buffers stay busy (vksift_isBufferAvailable), the accessors wait. The
   * SIFT buffers of the pairs must still hold the features that were matched. A new matching invalidates the results like it invalidates the filtered matches.
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued): no filtered matching to verify, nb_hypotheses 0 or above 65536, threshold_px not a positive finite number,
   * pair out of range. */
  typedef struct
  {
    float H[9];            /* row-major, pixel coordinates of A -> B, H[8] == 1 */
    uint32_t nb_matches;   /* filtered matches of the pair */
    uint32_t nb_inliers;
    uint32_t best_hypothesis;
    uint32_t valid;        /* 0: fewer than 4 matches, no hypothesis with 4 inliers, or a model that cannot be normalised; everything else is zero then */
  } vksift_ext_Homography; /* 52 bytes */
  VKSIFT_EXPORT void vksift_ext_verifyHomography(vksift_Instance instance, uint32_t nb_hypotheses, float threshold_px, uint64_t seed);
  VKSIFT_EXPORT void vksift_ext_getHomography(vksift_Instance instance, uint32_t pair, vksift_ext_Homography *out);
  /* vksift_ext_getFilteredMatchesNumber(pair) bytes, in the order of the filtered matches: 1 = inlier of the returned model */
  VKSIFT_EXPORT void vksift_ext_downloadInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask);
  /* The same for a fundamental matrix: "are these matches consistent with some rigid two-view geometry?". nb_hypotheses seven-point samples per pair from the
   * same generator; each gives up to three models (the real roots of the seven-point cubic, numbered in increasing order); a match is an inlier when its
   * Sampson distance is below threshold_px; the model with the most inliers wins, ties to the lowest (hypothesis, root). Deterministic, restated bit for bit by
   * tests/np_verify_f.py. Contract, busy buffers, errors and invalidation as for vksift_ext_verifyHomography. The two models keep separate results and masks:
   * after one vksift_ext_matchFeaturesFiltered both may be run and both read (each accessor is an error until its own model has been verified) — comparing the
   * two inlier counts is how a caller recognises a planar scene or a pure rotation, which this estimator does not handle (seven coplanar points do not
   * determine F). No rank or orientation test beyond the seven-point construction, no refit on the inliers in this call (F is the seven-point model of the
   * winning sample): vksift_ext_refineFundamental (below) refits it on the GPU. */
  typedef struct
  {
    float F[9];            /* row-major, pixel coordinates: (xb, yb, 1) F (xa, ya, 1)^T = 0; largest |entry| in [1, 2) */
    uint32_t nb_matches;   /* filtered matches of the pair */
    uint32_t nb_inliers;
    uint32_t best_hypothesis;
    uint32_t best_root;
    uint32_t valid;        /* 0: fewer than 7 matches, no model with 8 inliers, or a model that is not finite; everything else is zero then */
  } vksift_ext_Fundamental; /* 56 bytes */
  VKSIFT_EXPORT void vksift_ext_verifyFundamental(vksift_Instance instance, uint32_t nb_hypotheses, float threshold_px, uint64_t seed);
  VKSIFT_EXPORT void vksift_ext_getFundamental(vksift_Instance instance, uint32_t pair, vksift_ext_Fundamental *out);
  VKSIFT_EXPORT void vksift_ext_downloadFundamentalInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask);
  /* Time (ms) of the last verification of either model (its three launches + the result posting), HIP events; needs profiling on. -1 when there is none. */
  VKSIFT_EXPORT float vksift_ext_getVerifyTime(vksift_Instance instance);

  /* ---- GPU-side refit of the verified homographies on their inliers -----------------------------------------------------
   * The step between verification and guided matching: for every pair of the last vksift_ext_verifyHomography, nb_rounds (1 .. 8) locally optimised rounds in
   * one launch, without downloading matches, features or masks. A round fits a least-squares homography to the matches the current mask marks (conditioned
   * coordinates, a linear start, two Gauss-Newton steps on the forward transfer error, the error the inlier test measures) and scores all matches of the pair
   * again under the published model with the test of vksift_ext_matchFeaturesGuided at threshold_px; round r starts from the mask of round r - 1, the first from
   * the RANSAC mask. A round is accepted iff it can be computed and has at least as many inliers as the result kept so far; the first one that is not ends the
   * loop, so nb_inliers never falls below the verification's. rounds == 0: H, nb_inliers and the mask are the verification's (the mask byte for byte). A pair whose verification is not
   * valid: everything zero. Deterministic: every sum has a fixed order, tests/np_refine.py restates the estimator bit for bit.
   * Contract of guided matching: asynchronous, queued behind the matching and the verification, the pairs' buffers stay busy, the accessors wait; results of
   * its own (filtered matches, both verified models, their masks and the guided matches stay readable and unchanged), replaced by the next run, invalidated
   * by a new matching, plain or filtered, and by a new vksift_ext_verifyHomography (not by vksift_ext_verifyFundamental).
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, earlier refined results untouched): no verified homography, nb_rounds 0 or above 8, threshold_px not a
   * positive finite number or one whose square (threshold_px 2^-13)^2 2^26, the fp32 value the test compares with, is zero or not finite (below about 1e-19,
   * above about 1e19), pair out of range, out == NULL. */
  typedef struct
  {
    float H[9];            /* row-major, pixel coordinates of A -> B, H[8] == 1 */
    uint32_t nb_matches;   /* filtered matches of the pair */
    uint32_t nb_inliers;   /* >= the verification's */
    uint32_t rounds;       /* the last accepted round; 0: the verification's model, count and mask */
    uint32_t valid;        /* 0: the pair's verification is not valid; everything else is zero then */
  } vksift_ext_RefinedHomography; /* 52 bytes */
  VKSIFT_EXPORT void vksift_ext_refineHomography(vksift_Instance instance, uint32_t nb_rounds, float threshold_px);
  VKSIFT_EXPORT void vksift_ext_getRefinedHomography(vksift_Instance instance, uint32_t pair, vksift_ext_RefinedHomography *out);
  /* vksift_ext_getFilteredMatchesNumber(pair) bytes, in the order of the filtered matches: 1 = admissible under the refined model */
  VKSIFT_EXPORT void vksift_ext_downloadRefinedInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask);
  /* Time (ms) of the last vksift_ext_refineHomography (its launch + the result posting), HIP events; needs profiling on. -1 when there is none. */
  VKSIFT_EXPORT float vksift_ext_getRefineTime(vksift_Instance instance);
  /* The same for the fundamental matrices of the last vksift_ext_verifyFundamental: nb_rounds (1 .. 8) locally optimised rounds per pair in one launch. A
   * round needs at least eight marked matches and fits a least-squares F to them: conditioned coordinates, the entry of F that is largest in the model the
   * round starts from fixed to 1, a linear start, two steps reweighted by the Sampson denominator (so that the error minimised is the one the inlier test
   * measures), two Newton steps on the determinant for rank 2, published in the convention of vksift_ext_Fundamental; then all matches of the pair are scored
   * again under the published model with the test of vksift_ext_matchFeaturesGuided at threshold_px. Round r starts from the mask and the model of round r - 1,
   * the first from the verification's. Acceptance, rounds == 0, invalid pairs, determinism (tests/np_refine_f.py restates the estimator bit for bit), contract
   * and errors as for vksift_ext_refineHomography, with "no verified fundamental matrix" in place of "no verified homography". The two models keep separate
   * refined results: these are invalidated by a new matching, plain or filtered, and by a new vksift_ext_verifyFundamental, not by
   * vksift_ext_verifyHomography or vksift_ext_refineHomography, and vksift_ext_refineFundamental leaves the refined homographies alone.
   * Not attempted: no chirality test; no handling of the planar degeneracy (coplanar inliers give a near-singular system, and whatever model comes out is
   * subject to the acceptance rule like any other). */
  typedef struct
  {
    float F[9];            /* row-major, pixel coordinates: (xb, yb, 1) F (xa, ya, 1)^T = 0; largest |entry| in [1, 2) */
    uint32_t nb_matches;   /* filtered matches of the pair */
    uint32_t nb_inliers;   /* >= the verification's */
    uint32_t rounds;       /* the last accepted round; 0: the verification's model, count and mask */
    uint32_t valid;        /* 0: the pair's verification is not valid; everything else is zero then */
  } vksift_ext_RefinedFundamental; /* 52 bytes */
  VKSIFT_EXPORT void vksift_ext_refineFundamental(vksift_Instance instance, uint32_t nb_rounds, float threshold_px);
  VKSIFT_EXPORT void vksift_ext_getRefinedFundamental(vksift_Instance instance, uint32_t pair, vksift_ext_RefinedFundamental *out);
  /* vksift_ext_getFilteredMatchesNumber(pair) bytes, in the order of the filtered matches: 1 = admissible under the refined model */
  VKSIFT_EXPORT void vksift_ext_downloadRefinedFundamentalInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask);
  /* Time (ms) of the last vksift_ext_refineFundamental (vksift_ext_getRefineTime reports the homography's only). -1 when there is none. */
  VKSIFT_EXPORT float vksift_ext_getRefineFundamentalTime(vksift_Instance instance);

  /* ---- GPU-side guided matching -----------------------------------------------------------------------------------------
   * The step after a model is known: every feature of A is matched again against only those features of B that agree with the pair's model, so the ratio test
   * compares the best candidate with the second best among the geometrically possible ones, not with a look-alike elsewhere in the image (repeated structure),
   * for every pair of the last vksift_ext_matchFeaturesFiltered call, without downloading features or descriptors. With the model M (nine floats, row-major,
   * pixel coordinates) (a, b) is admissible under a homography iff, with (u, v, d) = M (xa, ya, 1), d > 0 and (u - xb d)^2 + (v - yb d)^2 < (d d) t2; under a
   * fundamental matrix iff, with l = M (xa, ya, 1), m = M^T (xb, yb, 1), r = (xb, yb, 1) l, r r < t2 ((l0 l0 + l1 l1) + (m0 m0 + m1 m1)); t2 = threshold_px^2;
   * fp32, every operation rounded once, in this order (tests/np_guided.py restates the records bit for bit). Among the admissible b the nearest and the second
   * nearest descriptor of a (exact integer distances, ties to the lowest index; padding rows are never candidates), and the same for every b over the admissible
   * a (the same relation: the model is not inverted). (a, b1) is kept iff dist1 <= max_distance (+inf: no limit), dist1 / dist2 < ratio (true without a second
   * candidate) and, with cross_check, b1's nearest admissible a is a and passes its own ratio test. Records in increasing idx_a; dist_a_b2 = +inf without a
   * second candidate. A pair whose model is not valid has no guided matches.
   * The test runs on the PUBLISHED model, so that a caller can reproduce it from public outputs and a supplied model means the same thing; the inlier masks
   * come from the scaled internal model: it is NOT promised that a filtered match is admissible exactly when its mask byte is 1, to the last bit.
   * models == NULL: the model of that kind verified for every pair of the last vksift_ext_matchFeaturesFiltered (an error if it has not been); otherwise 9
   * floats per pair, the caller's own models in the same convention, all finite; they are copied before the call returns. The refined homographies of
   * vksift_ext_refineHomography are handed over this way (the H[9] of vksift_ext_getRefinedHomography, pair by pair): their refined masks are exactly the
   * admissibility of the filtered matches under them. The refined fundamental matrices of vksift_ext_refineFundamental likewise (the F[9] of
   * vksift_ext_getRefinedFundamental with VKSIFT_EXT_GUIDE_FUNDAMENTAL), with the same guarantee.
   * Contract of the verification entry points: asynchronous, queued behind the matching and the verification, the pairs' buffers stay busy, the accessors wait;
   * results of its own (filtered matches, both models and their masks stay readable), replaced by the next run, invalidated by a new matching, plain or filtered.
   * Precondition, as for the verification: the buffers of the pairs still hold the features that were matched. A detection or an upload into one of them after
   * vksift_ext_matchFeaturesFiltered is not noticed: the row counts are the matching's, the rows the buffer's present ones, and the records are then
   * meaningless (every read stays inside the buffers' storage). Match again first.
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, earlier guided results untouched): no filtered matching, models == NULL for a model that has not been verified,
   * an unknown kind, threshold_px not positive and finite, ratio or max_distance not greater than 0, a supplied model that is not finite, pair out of range. */
#define VKSIFT_EXT_GUIDE_HOMOGRAPHY 0u
#define VKSIFT_EXT_GUIDE_FUNDAMENTAL 1u
  VKSIFT_EXPORT void vksift_ext_matchFeaturesGuided(vksift_Instance instance, uint32_t model, const float *models, float threshold_px, float ratio,
                                                    float max_distance, bool cross_check);
  VKSIFT_EXPORT uint32_t vksift_ext_getGuidedMatchesNumber(vksift_Instance instance, uint32_t pair);
  VKSIFT_EXPORT void vksift_ext_downloadGuidedMatches(vksift_Instance instance, uint32_t pair, vksift_ext_FilteredMatch *matches);
  /* Time (ms) of the last guided matching (gather + sweeps + decision + the count posting), HIP events; needs profiling on. -1 when there is none. */
  VKSIFT_EXPORT float vksift_ext_getGuidedMatchTime(vksift_Instance instance);

  /* ---- Multi-view feature tracks ------------------------------------------------------------------------------------------
   * The step every structure-from-motion or SLAM caller takes after the pair stages (COLMAP's correspondence graph, OpenMVG's TracksBuilder, OpenSfM's
   * create_tracks): the matches of ALL pairs of the last vksift_ext_matchFeaturesFiltered call are merged, and every connected set of features is one scene
   * point, a track — on the device, by a lock-free union-find over the results the pair stages left there, without one download of matches and masks per pair.
   * A node is (gpu_buffer_id, row), row in download order. The edges come from `source`: FILTERED and GUIDED take every record (idx_a, idx_b) of every pair p,
   * which joins (A[p], idx_a) and (B[p], idx_b); the four mask sources take the filtered records whose byte in that stage's mask is 1, of the pairs whose
   * record of that stage has valid != 0 (a pair whose model is not valid contributes no edge). A pair with A == B contributes edges like any other; an edge
   * with both ends on one node joins nothing. A track is a connected component of at least two nodes. Tracks are numbered from 0 in the order of their smallest
   * member, members compared by (gpu_buffer_id, row). vksift_ext_Track: gpu_buffer_id and row of the smallest member, length = the number of members,
   * nb_buffers = the number of distinct buffers among them. A track is CONFLICTING iff length > nb_buffers: two features of one image have been merged; callers
   * drop or split such tracks, the library only reports them. vksift_ext_TrackStats: nb_tracks; nb_conflicting; nb_features = the sum of the lengths; nb_edges =
   * the edges taken from the source, edges inside one buffer, on one node and duplicates included.
   * vksift_ext_downloadTracks writes nb_tracks records. vksift_ext_downloadFeatureTracks(b, out) writes vksift_getFeaturesNumber(b) words, the track number of
   * every row of b or VKSIFT_EXT_NO_TRACK; b must be a buffer of the pair list.
   * Deterministic: the same inputs give the same bytes on every run, whatever the scheduling; the numbering depends on nothing but the graph
   * (tests/np_tracks.py restates it).
   * Not attempted: no member list per track here (vksift_ext_selectTrackObservations, below, builds it); no splitting of conflicting tracks. (Tracks across
   * several matching calls: vksift_ext_beginTrackAccumulation, below.)
   * Contract of guided matching: asynchronous, queued on the instance stream behind the matching and whatever produced the source, the pairs' buffers stay
   * busy, the accessors wait; results of its own (every pair result stays readable and unchanged), replaced by the next vksift_ext_buildTracks, invalidated by
   * a new matching, plain or filtered. A verification or refit queued after a build does not touch the tracks already built. Precondition, as for guided
   * matching: the buffers of the pairs still hold the features that were matched (the row counts are the matching's).
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, earlier tracks untouched): no filtered matching, an unknown source, a source whose stage has not been run for
   * the present matching, out == NULL, a buffer outside the pair list, an accessor called before any build. A launch or allocation failure is
   * VKSIFT_VULKAN_ERROR. */
#define VKSIFT_EXT_TRACKS_FILTERED 0u   /* every filtered match of every pair */
#define VKSIFT_EXT_TRACKS_VERIFIED_H 1u /* matches whose byte in the verified homography's mask is 1 */
#define VKSIFT_EXT_TRACKS_VERIFIED_F 2u
#define VKSIFT_EXT_TRACKS_REFINED_H 3u
#define VKSIFT_EXT_TRACKS_REFINED_F 4u
#define VKSIFT_EXT_TRACKS_GUIDED 5u     /* the guided matches of every pair */
#define VKSIFT_EXT_NO_TRACK 0xFFFFFFFFu
  typedef struct
  {
    uint32_t gpu_buffer_id, row, length, nb_buffers;
  } vksift_ext_Track; /* 16 bytes */
  typedef struct
  {
    uint32_t nb_tracks, nb_conflicting, nb_features, nb_edges;
  } vksift_ext_TrackStats; /* 16 bytes */
  VKSIFT_EXPORT void vksift_ext_buildTracks(vksift_Instance instance, uint32_t source);
  VKSIFT_EXPORT void vksift_ext_getTrackStats(vksift_Instance instance, vksift_ext_TrackStats *out);
  VKSIFT_EXPORT void vksift_ext_downloadTracks(vksift_Instance instance, vksift_ext_Track *tracks);
  VKSIFT_EXPORT void vksift_ext_downloadFeatureTracks(vksift_Instance instance, uint32_t gpu_buffer_id, uint32_t *track_ids);
  /* Time (ms) of the last vksift_ext_buildTracks or vksift_ext_buildTracksAccumulated (its launches + the statistics' posting), HIP events; needs profiling
   * on. -1 when there is none. */
  VKSIFT_EXPORT float vksift_ext_getTracksTime(vksift_Instance instance);

  /* ---- Tracks across matching calls ---------------------------------------------------------------------------------------
   * A matching call takes at most batch_capacity pairs, and vksift_ext_buildTracks sees the pairs of the last call only. A view graph with more pairs goes
   * through a device-resident EDGE STORE that outlives a matching: begin once, match a chunk of the pair list and accumulate, as often as needed, then build.
   * ACCUMULATE(source) takes the edges vksift_ext_buildTracks(source) would take from the present matching — the same selection byte for byte: the source's
   * records, its mask bytes equal to 1, the pair's valid word, both rows stored — and appends them as vksift_ext_TrackEdge {A[p], idx_a, B[p], idx_b} behind
   * what the store holds, slot ascending and within a slot record ascending. max_edges is the store's capacity: positions at or beyond it are not written,
   * nb_dropped counts the edges that were not, nb_edges = min(total, max_edges); nb_calls counts the accumulate calls.
   * ROW TABLE: the store keeps one row count per SIFT buffer. The first call that names a buffer records the count the matching left for it (the word
   * vksift_ext_buildTracks reads, on the device: the host waits for nothing). A later call whose count for that buffer differs adds 1 to nb_changed_buffers
   * and leaves the table as it was: the precondition "the buffers still hold the features that were matched" is broken, and the caller can see it.
   * BEGIN empties the store and the row table and sets the capacity. Nothing else clears the store: not a new matching, verification, refit or guided
   * matching, not a build of either kind.
   * BUILD computes the tracks of the graph whose nodes are the stored rows — those below min(table[b], max_nb_sift_per_buffer) — of every buffer b the
   * store's calls named and whose edges are the store's; an edge that names a row that is not stored is no edge. Numbering, vksift_ext_Track,
   * vksift_ext_TrackStats and the per-feature words are exactly those of vksift_ext_buildTracks; nb_edges counts the store's edges that were taken. The result
   * REPLACES the instance's tracks: vksift_ext_getTrackStats, vksift_ext_downloadTracks, vksift_ext_downloadFeatureTracks (for every buffer the store's
   * calls named; it writes min(table[b], max_nb_sift_per_buffer) words, the count of the first call that named b), vksift_ext_selectTrackObservations and everything behind it serve it unchanged. It is invalidated where tracks are, by a new matching or a
   * new build of either kind; the store survives, so a caller who matches again simply builds again.
   * EQUIVALENCE: one accumulate followed by one build gives, byte for byte, what vksift_ext_buildTracks(source) gives for the same matching.
   * Deterministic (tests/np_track_edges.py restates the rule).
   * Not attempted: edges are not de-duplicated; a single edge or call cannot be removed; conflicting tracks are not split; the store does not grow.
   * Contract of vksift_ext_buildTracks: asynchronous on the instance stream, the accessors wait, every pair result stays readable and byte-identical. Busy
   * buffers: an accumulate keeps the pairs' buffers busy; the accumulated build and every stage that reads its tracks keep ALL participating buffers busy,
   * not only those of the last pair list.
   * Memory: 16 bytes per edge of max_edges. vksift_ext_beginTrackAccumulation waits for everything the instance has in flight; since an accumulation can
   * involve every buffer, the first begin of an instance with 2 batch_capacity < sift_buffer_count releases the storage of the tracks, observations, points
   * and view index (and invalidates those results), which from then on is allocated for sift_buffer_count buffers instead of 2 batch_capacity: per node
   * (buffer x max_nb_sift_per_buffer) 32 bytes for the tracks, about 48 for the observations, 16 for the points and about 37 for the view index, scratch included. An instance with
   * 2 batch_capacity >= sift_buffer_count releases nothing.
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, the store untouched): max_edges == 0, accumulate or build with no accumulation begun, accumulate with no
   * filtered matching, an unknown source, a source whose stage has not been run for the present matching, build before any accumulate, out == NULL, an
   * accessor called before begin. A launch or allocation failure is VKSIFT_VULKAN_ERROR; after it every entry but begin refuses the store. */
  typedef struct
  {
    uint32_t gpu_buffer_id_a, row_a, gpu_buffer_id_b, row_b;
  } vksift_ext_TrackEdge; /* 16 bytes */
  typedef struct
  {
    uint32_t nb_edges, nb_dropped, nb_calls, nb_changed_buffers;
  } vksift_ext_TrackEdgeStats; /* 16 bytes */
  VKSIFT_EXPORT void vksift_ext_beginTrackAccumulation(vksift_Instance instance, uint32_t max_edges);
  VKSIFT_EXPORT void vksift_ext_accumulateTrackEdges(vksift_Instance instance, uint32_t source); /* the VKSIFT_EXT_TRACKS_* sources */
  VKSIFT_EXPORT void vksift_ext_getTrackEdgeStats(vksift_Instance instance, vksift_ext_TrackEdgeStats *out);
  VKSIFT_EXPORT void vksift_ext_downloadTrackEdges(vksift_Instance instance, vksift_ext_TrackEdge *edges); /* nb_edges records */
  VKSIFT_EXPORT void vksift_ext_buildTracksAccumulated(vksift_Instance instance);
  /* Time (ms) of the last vksift_ext_accumulateTrackEdges (table upload + launches + the statistics' posting), HIP events; needs profiling on. -1 when there
   * is none. */
  VKSIFT_EXPORT float vksift_ext_getAccumulateTime(vksift_Instance instance);

  /* ---- GPU-side track observations ----------------------------------------------------------------------------------------
   * What triangulation and bundle adjustment read: the table track -> [(image, feature, x, y)] of the tracks a caller keeps, built on the device from the
   * tracks of the last vksift_ext_buildTracks, in two or three downloads however many buffers took part — instead of one word array and every 164-byte feature
   * record per buffer, a host sort and a host filter (OpenMVG's TracksBuilder::Filter, OpenSfM's min_track_length, COLMAP's track-length options).
   * Input: the tracks of the last vksift_ext_buildTracks.
   * Selection: track t is selected iff length >= min_length, and (max_length == 0 or length <= max_length), and (conflicts ==
   * VKSIFT_EXT_OBS_KEEP_CONFLICTING or length == nb_buffers).
   * Rejection counts: nb_rejected_length counts the tracks that fail the length test, nb_rejected_conflicting those that pass it and are dropped as
   * conflicting; nb_tracks + nb_rejected_length + nb_rejected_conflicting == vksift_ext_TrackStats.nb_tracks.
   * Numbering: selected tracks keep their relative order, which is that of their smallest member; track_ids[m] is the number of selected track m in
   * vksift_ext_downloadTracks.
   * Layout: offsets[m] .. offsets[m+1] are the observations of selected track m; offsets[0] == 0 and offsets[nb_tracks] == nb_observations; inside a track
   * the members come in increasing (gpu_buffer_id, row).
   * Positions: x, y are the first two floats of the stored feature at that row (download order), bit for bit.
   * Deterministic: the same inputs give the same bytes on every run, whatever the scheduling (tests/np_observations.py restates the rule).
   * With no selected track, offsets is the single word 0.
   * Not attempted: no splitting of conflicting tracks, no threshold on nb_buffers. (The observations of one image: vksift_ext_indexObservationsByView, below.)
   * Contract of vksift_ext_buildTracks: asynchronous, queued on the instance stream behind the build, the pairs' buffers stay busy until it has run, the
   * accessors wait; results of its own (the tracks and every pair result stay readable and byte-identical), replaced by the next
   * vksift_ext_selectTrackObservations, invalidated by a new vksift_ext_buildTracks and by a new matching, plain or filtered. Precondition, as for guided
   * matching: the buffers of the pairs still hold the features that were matched.
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, earlier observations untouched): no tracks built for the present matching, min_length < 2, max_length neither 0
   * nor >= min_length, an unknown conflicts, out == NULL, an accessor called before any selection. A launch or allocation failure is VKSIFT_VULKAN_ERROR. */
#define VKSIFT_EXT_OBS_KEEP_CONFLICTING 0u
#define VKSIFT_EXT_OBS_DROP_CONFLICTING 1u /* tracks with length > nb_buffers are not selected */
  typedef struct
  {
    uint32_t gpu_buffer_id, row;
    float x, y;
  } vksift_ext_Observation; /* 16 bytes */
  typedef struct
  {
    uint32_t nb_tracks, nb_observations, nb_rejected_length, nb_rejected_conflicting;
  } vksift_ext_ObservationStats; /* 16 bytes */
  VKSIFT_EXPORT void vksift_ext_selectTrackObservations(vksift_Instance instance, uint32_t min_length, uint32_t max_length, uint32_t conflicts);
  VKSIFT_EXPORT void vksift_ext_getObservationStats(vksift_Instance instance, vksift_ext_ObservationStats *out);
  VKSIFT_EXPORT void vksift_ext_downloadObservationOffsets(vksift_Instance instance, uint32_t *offsets);     /* nb_tracks + 1 words */
  VKSIFT_EXPORT void vksift_ext_downloadObservationTrackIds(vksift_Instance instance, uint32_t *track_ids);  /* nb_tracks words */
  VKSIFT_EXPORT void vksift_ext_downloadObservations(vksift_Instance instance, vksift_ext_Observation *obs); /* nb_observations records */
  /* Time (ms) of the last vksift_ext_selectTrackObservations (its launches + the statistics' posting), HIP events; needs profiling on. -1 when there is none. */
  VKSIFT_EXPORT float vksift_ext_getObservationsTime(vksift_Instance instance);

  /* ---- GPU-side triangulation of the selected tracks ----------------------------------------------------------------------
   * One 3-D point per selected track of the last vksift_ext_selectTrackObservations, under cameras the caller knows (a calibrated rig, odometry, poses with
   * priors: COLMAP's point_triangulator, OpenMVG's ComputeStructureFromKnownPoses, OpenSfM's triangulation of shots with priors), where the table lies on the
   * device: nothing is downloaded or uploaded except the camera table, and a table of 32-byte points leaves the device instead of the observations.
   * Cameras: 12 floats per SIFT buffer of the instance, indexed by gpu_buffer_id, a row-major 3x4 P. With (u, v, w) = P (X, Y, Z, 1) the pixel is (u / w,
   * v / w); w > 0 means the point is in front of the camera. Only the cameras of the buffers that took part in the last vksift_ext_buildTracks are read; those
   * must be finite. The cameras are copied before the call returns. Precondition (stated, not checked): the left 3x3 block has a positive determinant, so
   * that P = K [R | t].
   * Point m belongs to selected track m of the observation table. status is 0 for an accepted point, otherwise all the flags that apply;
   * cos_min_angle >= 1 switches the angle test off. nb_accepted + nb_failed + nb_rejected == nb_points == vksift_ext_ObservationStats.nb_tracks.
   * THE RULE, per selected track with members i = 0 .. n-1 in table order. Arithmetic is fp32 add, subtract, multiply, divide and sqrtf, each rounded once, in
   * a written order, with no fmaf (the order is spelled out at vksift_hip_triangulate_tracks in vksift_hip.h; tests/np_triangulate.py restates it bit for bit).
   *  1 Bearings: with rows m1, m2, m3 of the left 3x3 block, b_i = x_i (m2 x m3) + y_i (m3 x m1) + (m1 x m2), scaled by 1 / sqrtf(b.b). min_cos is the minimum
   *    of b_i . b_j over all i < j.
   *  2 Linear start: each member gives the rows x_i P3 - P1 and y_i P3 - P2, each scaled by 1 / sqrtf of the squared length of its first three entries; the
   *    3x3 normal equations of the inhomogeneous solution (X, Y, Z, 1) are solved by Gauss-Jordan with the refits' pivot rule (rows below compared in turn by
   *    |entry| bit pattern, the row multiplied by 1 / pivot).
   *  3 Up to two Gauss-Newton steps on the summed squared reprojection error (residuals u/w - x and v/w - y, analytic Jacobian, the same 3x3 solve). A step is
   *    accepted iff it can be computed (every w normal and finite, every pivot usable, the new point finite) and the cost at the new point is not larger
   *    than at the old one; the first step that is not accepted ends the loop.
   *  4 Scoring at the final X: max_sq_error is the largest (u/w - x)^2 + (v/w - y)^2; BEHIND iff some w <= 0; ERROR iff not max_sq_error < threshold_px^2;
   *    ANGLE iff cos_min_angle < 1 and not min_cos < cos_min_angle; DEGENERATE when a bearing, a row scale, a pivot or the start cannot be computed or is not
   *    finite (a scale or pivot that is zero, subnormal or not finite), or a member names a buffer without a camera.
   *  5 Sums over members have one order whatever the scheduling: a group of G = 16 lanes owns a track, lane j adds members j, j + 16, ... in increasing
   *    order, the lanes are then added by the refits' xor butterfly (offsets 8, 4, 2, 1). G is part of the rule.
   * Deterministic: the same inputs give the same bytes on every run.
   * Not attempted: no removal of single outlying observations (a track is taken or left whole); no joint bundle adjustment and no camera from scratch (the
   * cameras are refined on these points, the points held fixed, by vksift_ext_refineCameras, below: the two calls alternate); no conditioning of the world
   * frame — the arithmetic is fp32, so a caller puts the origin near the scene.
   * Contract of vksift_ext_selectTrackObservations: asynchronous, queued on the instance stream behind the selection, the pairs' buffers stay busy until it
   * has run, the accessors wait; results of its own (tracks, observations and every pair result stay readable and byte-identical), replaced by the next
   * vksift_ext_triangulateTracks, invalidated wherever the observations are: by a new selection, a new vksift_ext_buildTracks, a new matching. Failures as
   * stated at vksift_ext_matchFeaturesBatch.
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, earlier points untouched): no observations selected for the present tracks, cameras == NULL, a camera that is
   * read is not finite, threshold_px not positive and finite or its fp32 square zero or not finite, cos_min_angle NaN, out == NULL, an accessor called
   * before any triangulation. A launch or allocation failure is VKSIFT_VULKAN_ERROR. */
#define VKSIFT_EXT_POINT_DEGENERATE 1u /* no solution: see the rule; X = 0 and every other field but nb_observations is 0 */
#define VKSIFT_EXT_POINT_TOO_LONG 2u   /* more than VKSIFT_EXT_TRIANGULATE_MAX_OBSERVATIONS members: not computed, fields as for DEGENERATE */
#define VKSIFT_EXT_POINT_BEHIND 4u     /* some observation has w <= 0 at X */
#define VKSIFT_EXT_POINT_ERROR 8u      /* max_sq_error is not below threshold_px^2 */
#define VKSIFT_EXT_POINT_ANGLE 16u     /* min_cos is not below cos_min_angle */
#define VKSIFT_EXT_TRIANGULATE_MAX_OBSERVATIONS 1024u
  typedef struct
  {
    float X[3];         /* world coordinates */
    float max_sq_error; /* largest squared reprojection error over the members, pixels^2 */
    float min_cos;      /* smallest cosine between two members' bearing rays: the largest triangulation angle */
    uint32_t status;    /* 0: accepted; otherwise the flags above, all that apply */
    uint32_t steps;     /* accepted Gauss-Newton steps, 0 .. 2 */
    uint32_t nb_observations;
  } vksift_ext_Point; /* 32 bytes; point m belongs to selected track m of the observation table */
  typedef struct
  {
    uint32_t nb_points, nb_accepted, nb_failed /* DEGENERATE or TOO_LONG */, nb_rejected /* computed, some of BEHIND / ERROR / ANGLE */;
  } vksift_ext_PointStats; /* 16 bytes */
  VKSIFT_EXPORT void vksift_ext_triangulateTracks(vksift_Instance instance, const float *cameras, float threshold_px, float cos_min_angle);
  VKSIFT_EXPORT void vksift_ext_getPointStats(vksift_Instance instance, vksift_ext_PointStats *out);
  VKSIFT_EXPORT void vksift_ext_downloadPoints(vksift_Instance instance, vksift_ext_Point *points); /* nb_points records */
  /* Time (ms) of the last vksift_ext_triangulateTracks (the camera upload, its launches + the statistics' posting), HIP events; needs profiling on. -1 when there is none. */
  VKSIFT_EXPORT float vksift_ext_getTriangulateTime(vksift_Instance instance);

  /* ---- GPU-side per-view index of the observation table -------------------------------------------------------------------
   * The observation table of the last vksift_ext_selectTrackObservations inverted by view — the observations of one image, each with the number of its
   * selected track —, on the device: what camera refinement, resection and any per-image pass over the tracks read, without a download and a host sort of the
   * table by gpu_buffer_id.
   * view_offsets has sift_buffer_count + 1 words, indexed by gpu_buffer_id: records view_offsets[b] .. view_offsets[b+1] are the observations of buffer b
   * (none for a buffer that took no part); view_offsets[0] == 0 and view_offsets[sift_buffer_count] == nb_observations ==
   * vksift_ext_ObservationStats.nb_observations. Inside a view the records are in table order: increasing point — the number m of the selected track, which
   * is also the number of its vksift_ext_Point —, the two members of a conflicting track in one view in increasing row. x, y are copied bit for bit.
   * Deterministic: a stable radix sort keyed on the buffer, linear in the observations, no atomics on global memory; the same inputs give the same bytes on
   * every run (tests/np_cameras.py restates the rule, vksift_hip_index_views in vksift_hip.h spells it out).
   * Contract of vksift_ext_selectTrackObservations: asynchronous, queued on the instance stream behind the selection, the pairs' buffers stay busy until it
   * has run, the accessors wait; results of its own (tracks, observations, points and every pair result stay readable and byte-identical), replaced by the
   * next index, invalidated wherever the observations are: by a new selection, a new vksift_ext_buildTracks, a new matching.
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, an earlier index untouched): no observations selected for the present tracks, out == NULL, an accessor called
   * before any index. A launch or allocation failure is VKSIFT_VULKAN_ERROR. */
  typedef struct
  {
    uint32_t point, row; /* the selected track (= point) number m, and the feature's row in its buffer */
    float x, y;
  } vksift_ext_ViewObservation; /* 16 bytes */
  typedef struct
  {
    uint32_t nb_views /* buffers with at least one observation */, nb_observations, largest_view, reserved /* 0 */;
  } vksift_ext_ViewStats; /* 16 bytes */
  VKSIFT_EXPORT void vksift_ext_indexObservationsByView(vksift_Instance instance);
  VKSIFT_EXPORT void vksift_ext_getViewStats(vksift_Instance instance, vksift_ext_ViewStats *out);
  VKSIFT_EXPORT void vksift_ext_downloadViewOffsets(vksift_Instance instance, uint32_t *view_offsets);                 /* sift_buffer_count + 1 words */
  VKSIFT_EXPORT void vksift_ext_downloadViewObservations(vksift_Instance instance, vksift_ext_ViewObservation *obs); /* nb_observations records */
  /* Time (ms) of the last vksift_ext_indexObservationsByView (its launches + the statistics' posting), HIP events; needs profiling on. -1 when there is none. */
  VKSIFT_EXPORT float vksift_ext_getIndexViewsTime(vksift_Instance instance);

  /* ---- GPU-side camera refinement on the triangulated points ---------------------------------------------------------------
   * The motion half of resection-intersection bundle adjustment, where vksift_ext_triangulateTracks is the structure half: every camera that took part in
   * the last vksift_ext_buildTracks refined on the accepted points of its view, the points held fixed, by up to nb_steps (1 .. 8) Gauss-Newton steps on the
   * summed squared reprojection error. Input: the view index (built first if the present observation table has none), the points of the last
   * vksift_ext_triangulateTracks and the camera table that call copied to the device; nothing is uploaded. Output: one record per SIFT buffer, indexed by
   * gpu_buffer_id. The refined P goes back into vksift_ext_triangulateTracks as it is: that is the alternation. Every participating camera is refined; the
   * caller keeps the input camera of whichever it wants fixed.
   * THE RULE, per view with the members of its index range in order. Arithmetic is fp32 add, subtract, multiply and divide, each rounded once, in a written
   * order, with no fmaf (the order is spelled out at vksift_hip_refine_cameras in vksift_hip.h; tests/np_cameras.py restates it bit for bit).
   *  1 A member is USED iff the status of its point is 0. Fewer than VKSIFT_EXT_CAMERA_MIN_OBSERVATIONS used members: TOO_FEW.
   *  2 At a camera P every used member gives the residuals u/w - x, v/w - y and their Jacobian rows with respect to a rigid motion of the world
   *    (omega, tau): (X x j, j) with j the triangulation's Jacobian row; the cost, the 6x6 normal equations and their right-hand side are summed.
   *  3 A step solves N d = -g by Gauss-Jordan with the refits' pivot rule, forms the Cayley rotation C of omega = d[0..2] — rational in omega, so no sine or
   *    cosine is needed — and P' = P [[C, tau], [0, 1]]: a right-multiplied rigid update keeps P = K [R | t] with the same K without ever decomposing P. The
   *    step is accepted iff it can be computed (every w normal and finite, every pivot usable, P' finite) and cost(P') <= cost(P); the first step that is not
   *    accepted ends the loop.
   *  4 Sums over members have one order whatever the scheduling: a workgroup of 256 lanes owns a view, lane j adds members j, j + 256, ... in increasing
   *    order, the lanes are added by the refits' block sum. The 256 is part of the rule.
   * nb_views == nb_refined + nb_unchanged + nb_failed. Deterministic: the same inputs give the same bytes on every run.
   * Not attempted: no estimation of K; no camera from scratch (no minimal solver, no RANSAC: the input camera must be close enough for Gauss-Newton); no
   * joint solve of cameras and points (the two halves alternate); no gauge fixing (refining all cameras lets the frame drift with the points: keep some input
   * cameras to pin it); no conditioning of the world frame — the arithmetic is fp32, so a caller keeps the origin near the scene, as for triangulation.
   * Contract of vksift_ext_triangulateTracks: asynchronous, queued on the instance stream behind the triangulation, the pairs' buffers stay busy until it has
   * run, the accessors wait; results of its own (tracks, observations, points and every pair result stay readable and byte-identical), replaced by the next
   * vksift_ext_refineCameras, invalidated wherever the points are — by a new selection, a new vksift_ext_buildTracks, a new matching — and by a new
   * vksift_ext_triangulateTracks, whose points and cameras they would no longer refer to.
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, earlier results untouched): no triangulation for the present observations, nb_steps 0 or above
   * VKSIFT_EXT_CAMERA_MAX_STEPS, out == NULL, an accessor called before any refinement. A launch or allocation failure is VKSIFT_VULKAN_ERROR. */
#define VKSIFT_EXT_CAMERA_ABSENT 1u     /* the buffer took no part in the last build: every other field is 0 */
#define VKSIFT_EXT_CAMERA_TOO_FEW 2u    /* fewer than VKSIFT_EXT_CAMERA_MIN_OBSERVATIONS used observations: P is the input camera, the costs and steps are 0 */
#define VKSIFT_EXT_CAMERA_DEGENERATE 4u /* the cost at the input camera cannot be computed (some w zero, subnormal or not finite, or a cost that is not finite): as TOO_FEW */
#define VKSIFT_EXT_CAMERA_BEHIND 8u     /* some used observation has w <= 0 at the final camera */
#define VKSIFT_EXT_CAMERA_MIN_OBSERVATIONS 6u
#define VKSIFT_EXT_CAMERA_MAX_STEPS 8u
  typedef struct
  {
    float P[12];              /* row-major 3x4: the refined camera, or the input camera where no step was accepted */
    float cost_start, cost;   /* summed squared reprojection error over the used observations, before and after */
    float max_sq_error;       /* largest squared error at the final camera */
    uint32_t nb_observations; /* used observations */
    uint32_t steps;           /* accepted steps, 0 .. nb_steps */
    uint32_t status;          /* 0, or the flags above */
  } vksift_ext_RefinedCamera; /* 72 bytes */
  typedef struct
  {
    uint32_t nb_views /* not ABSENT */, nb_refined /* steps > 0 */, nb_unchanged /* status 0 or BEHIND only, steps 0 */, nb_failed /* TOO_FEW or DEGENERATE */;
  } vksift_ext_CameraStats; /* 16 bytes */
  VKSIFT_EXPORT void vksift_ext_refineCameras(vksift_Instance instance, uint32_t nb_steps);
  VKSIFT_EXPORT void vksift_ext_getCameraStats(vksift_Instance instance, vksift_ext_CameraStats *out);
  VKSIFT_EXPORT void vksift_ext_downloadRefinedCameras(vksift_Instance instance, vksift_ext_RefinedCamera *cameras); /* sift_buffer_count records */
  /* Time (ms) of the last vksift_ext_refineCameras (the index where the call built it, its launches + the statistics' posting), HIP events; needs profiling
   * on. -1 when there is none. */
  VKSIFT_EXPORT float vksift_ext_getRefineCamerasTime(vksift_Instance instance);

  /* ---- GPU-side feature budget ------------------------------------------------------------------------------------------
   * Every SIFT buffer of [first_gpu_buffer_id, first_gpu_buffer_id + count) keeps its max_features strongest features (OpenCV's nfeatures, SiftGPU's -tc,
   * PopSift's --filter-max-extrema), selected and compacted on the device: no download, host sort and upload. The capacity max_nb_sift_per_buffer drops the
   * tail of a full section in raster order, wherever the features sit in the image; this call chooses by strength. Everything behind it is priced by the row
   * count (the matcher is N_A x N_B, the guided sweep visits all pairs, a download moves every stored record), so it goes between detection and matching.
   * With rows numbered in download order, key(row) is the 32 bits of the feature's `intensity` field with the sign bit cleared, compared as an unsigned integer:
   * |DoG response| for every finite value, and a total order on every bit pattern (-0 equals +0, infinities rank above finite values, NaN patterns above
   * those). The first min(n, max_features) rows by (key descending, row ascending) are kept, in download order: vksift_getFeaturesNumber becomes min(n,
   * max_features), vksift_downloadFeatures returns the kept records as they were, and a matching sees those rows. Deterministic. The orientations of one
   * keypoint are separate features with equal keys: a tie at the threshold is broken by row, so the budget may keep some of them and not the others.
   * A buffer that holds at most max_features features is not touched at all (its records, their order and its count; of what the instance keeps about it
   * only vksift_ext_getPlacedKeypointsNumber changes, which reads 0 after every budget call); selecting again with the same budget changes nothing. A detected buffer stays
   * laid out in its octave sections (the kept features of an octave stay in it), an uploaded one stays one dense run.
   * Contract of vksift_detectFeatures: asynchronous, queued on the instance stream behind every detection and matching already queued (staged plain
   * detections are launched first); the buffers are busy (vksift_isBufferAvailable false) until it has run, and every accessor of them waits for it.
   * Precondition on earlier results, as for the guided matching: filtered matches, verified or refined models and guided matches of an earlier matching
   * index the buffers' old rows. The selection is not noticed by them: the row counts are the matching's, the rows the buffer's present ones, and the
   * records are then meaningless (every read stays inside the buffers' storage). Match again first.
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, nothing changed): count 0 or above 512, a range outside sift_buffer_count, max_features 0. A launch failure
   * is VKSIFT_VULKAN_ERROR. */
  VKSIFT_EXPORT void vksift_ext_keepStrongestFeatures(vksift_Instance instance, uint32_t first_gpu_buffer_id, uint32_t count, uint32_t max_features);
  /* Time (ms) of the last vksift_ext_keepStrongestFeatures (its launches), HIP events; needs profiling on. -1 when there is none. */
  VKSIFT_EXPORT float vksift_ext_getKeepStrongestTime(vksift_Instance instance);

  /* ---- GPU-side feature budget, spread over the image --------------------------------------------------------------------
   * vksift_ext_keepStrongestFeatures ranks the whole image, which on real frames leaves the kept features on the most textured region. This call pairs the
   * count limit with a spatial rule (PopSift's --filter-grid, AliceVision's gridFiltering, OpenCV's GridAdaptedFeatureDetector, ORB-SLAM's bucketing): the
   * frame of image_width x image_height pixels is cut into grid_cols x grid_rows cells and every cell keeps its own strongest features first.
   * The cell of a feature: column bound j (1 <= j < grid_cols) is (float)((double)j * image_width / grid_cols), row bound j likewise from image_height and
   * grid_rows; the feature's column is the number of column bounds its x is at or above, its row likewise from y. Only comparisons take place: a NaN or a
   * negative coordinate falls into column / row 0, anything at or beyond the last bound into the last one, -0.0 is 0.0. An uploaded buffer carries no image
   * size, so the caller names it; it need not be the size of the detected image.
   * The rule, with key(row) and the row numbers of vksift_ext_keepStrongestFeatures, C = grid_cols * grid_rows and q = max_features / C (integer division):
   * a buffer of at most max_features features is not touched at all. Otherwise every cell keeps the first min(n_cell, q) of its rows by (key descending, row
   * ascending); then, among the rows not kept so far, the first max_features - (rows kept so far) by (key descending, row ascending) are kept as well. Exactly
   * max_features features remain: max_features is the TOTAL per buffer, not a number per cell; cells with fewer than q features pass their share on to the
   * strongest features elsewhere, and every cell that held at least q features keeps at least q. A 1 x 1 grid is vksift_ext_keepStrongestFeatures byte for
   * byte, and so is any grid with max_features < C (q = 0). Selecting again with the same arguments changes nothing. tests/np_spread.py restates the rule.
   * In every other respect — the kept features stay in download order and in their octave sections, asynchronous queueing behind staged detections, busy
   * buffers, accessors that wait, the precondition on earlier matching results — the contract is that of vksift_ext_keepStrongestFeatures.
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, nothing changed): whatever vksift_ext_keepStrongestFeatures refuses, image_width or image_height 0, grid_cols
   * or grid_rows 0 or above 16. A launch failure is VKSIFT_VULKAN_ERROR. */
  VKSIFT_EXPORT void vksift_ext_keepStrongestFeaturesGrid(vksift_Instance instance, uint32_t first_gpu_buffer_id, uint32_t count, uint32_t max_features,
                                                          uint32_t image_width, uint32_t image_height, uint32_t grid_cols, uint32_t grid_rows);
  /* Time (ms) of the last vksift_ext_keepStrongestFeaturesGrid (its launches), HIP events; needs profiling on. -1 when there is none. A timer of its own:
   * vksift_ext_getKeepStrongestTime reports the plain budget only. */
  VKSIFT_EXPORT float vksift_ext_getKeepStrongestGridTime(vksift_Instance instance);

  /* ---- RootSIFT descriptors ------------------------------------------------------------------------------------------------
   * The descriptors of every feature of the SIFT buffers [first_gpu_buffer_id, first_gpu_buffer_id + count) are converted to RootSIFT (Arandjelovic &
   * Zisserman 2012: COLMAP's default L1_ROOT normalisation, PopSift's --root-sift, the two lines most OpenCV callers write after detectAndCompute) in
   * place on the device: no download, conversion on the host and upload into another buffer. A descriptor d[0..127] with s = the sum of its bytes becomes
   * out[i] = min(255, round-half-up(512 sqrt(d[i] / s))), taken exactly — r is the integer with (2r - 1)^2 s <= 2^20 d[i] < (2r + 1)^2 s; integer
   * arithmetic decides, not a float rounding —, and an all-zero descriptor stays all zero. A bin is zero afterwards iff it was zero. The Euclidean
   * distance of two converted descriptors is the Hellinger distance of the originals; their norm is that of SIFT descriptors (about 512), so the
   * matcher, the ratio test, the verification, the refits and the guided matching take them as they are. Of a feature only the 128 descriptor bytes
   * change: x, y, the scales, sigma, orientation and intensity keep every bit, vksift_getFeaturesNumber its value, a detected buffer its octave
   * sections, an uploaded one its dense run, vksift_ext_getPlacedKeypointsNumber its count. The feature budget's key is untouched: budget, then
   * convert, and convert, then budget, give the same bytes.
   * The call converts whatever the buffers hold. It is NOT idempotent: two calls convert twice. The instance does not track which form a buffer is
   * in — that is the caller's to know; a detection, a describe call or an upload into the buffer makes it what they store. Matching a converted
   * buffer against an unconverted one is defined (exact distances between the rows as they are) and meaningless.
   * Contract of vksift_detectFeatures, as for vksift_ext_keepStrongestFeatures: asynchronous, queued on the instance stream behind every detection,
   * selection and matching already queued (staged plain detections are launched first); the buffers are busy (vksift_isBufferAvailable false) until
   * it has run, and every accessor of them waits for it: vksift_downloadFeatures and vksift_ext_exportDescriptorsDevice return converted descriptors,
   * a matching queued afterwards sees them.
   * Earlier results: matches, filtered matches, verified or refined models and guided matches of an earlier matching stay valid as indices — the
   * rows have not moved — but their distances are those of the old descriptors. Match again.
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, nothing changed): count 0 or above 512, a range outside sift_buffer_count. A launch failure is
   * VKSIFT_VULKAN_ERROR. */
  VKSIFT_EXPORT void vksift_ext_convertToRootSift(vksift_Instance instance, uint32_t first_gpu_buffer_id, uint32_t count);
  /* Time (ms) of the last vksift_ext_convertToRootSift (its launches), HIP events; needs profiling on. -1 when there is none. */
  VKSIFT_EXPORT float vksift_ext_getRootSiftTime(vksift_Instance instance);

  /* ---- Describe caller-supplied keypoints ---------------------------------------------------------------------------------
   * OpenCV's detectAndCompute(useProvidedKeypoints = true), SiftGPU's SetKeypointList, VLFeat's vl_sift with frames: the scale-space of the image is
   * built as for a detection, and the caller's keypoints take the place of the extraction stage. Keypoint (x, y, sigma) in image pixels goes to the octave and
   * scale a detection would have found it at — the inverse of sigma = seed_scale_sigma 2^(s / S) 2^octave, s rounded to the nearest scale, a comparison
   * against S + 1 thresholds (float)(seed_scale_sigma 2^((j + 0.5) / S)); beyond either end of the scale-space it takes the first or the last octave — at
   * scale_x = x 2^-octave, exactly. A keypoint is described iff x, y and sigma are finite, sigma 2^-octave lies in [0.02, 29], 0 <= scale_x < octave width and
   * 0 <= scale_y < octave height and, in GIVEN mode, 0 <= orientation <= 2 pi; the others are skipped without a word (tests/np_describe.py restates the rule
   * bit for bit).
   * mode VKSIFT_EXT_DESCRIBE_ORIENT: orientations from the image, as in a detection (a keypoint with several histogram peaks yields several features, the
   * supplied orientation is ignored). VKSIFT_EXT_DESCRIBE_GIVEN: the supplied orientation, exactly one feature per stored keypoint.
   * The buffer afterwards is an ordinary detected buffer, laid out in octave sections: downloads, matching, vksift_ext_keepStrongestFeatures (whose key is
   * `response`) and vksift_ext_exportDescriptorsDevice work on it unchanged. Download order: by octave, in each octave the keypoints in input order, then the
   * orientation copies. A feature carries x, y, sigma and response (its intensity field) of its keypoint bit for bit: that is how the caller joins the
   * features to its list. An octave's section holds its share of max_nb_sift_per_buffer as after a detection; keypoints beyond it are dropped in input order.
   * vksift_ext_getPlacedKeypointsNumber: the keypoints of the buffer's last describe call that were stored, before orientation copies; waits like
   * vksift_getFeaturesNumber. 0 once something else has filled the buffer, and once vksift_ext_keepStrongestFeatures or ...Grid has named it, whether or
   * not that call cut anything (when it is queued the host need not know yet how many features the buffer holds, so the count ends with the call, not
   * with its outcome); vksift_ext_convertToRootSift keeps it.
   * Contract of vksift_detectFeatures / vksift_ext_detectFeaturesBatch: asynchronous, the buffers busy until it has run, the accessors wait; images and
   * keypoints are copied before the call returns; the scale-space accessors show the described image afterwards (image 0 of a batch). Never deferred, never
   * replayed from a graph; the detect timings (vksift_ext_getDetectTimings) keep reporting the last detection.
   * Batch: image i takes the next nb_kps[i] keypoints of kps and SIFT buffer first_gpu_buffer_id + i.
   * VKSIFT_INVALID_INPUT_ERROR (nothing queued, nothing changed): whatever the detection entry points refuse, kps == NULL with a non-zero count, nb_kps == NULL
   * (batch), a count above max_nb_sift_per_buffer, an unknown mode. */
  typedef struct
  {
    float x, y, sigma, orientation, response;
  } vksift_ext_Keypoint;
#define VKSIFT_EXT_DESCRIBE_ORIENT 0u
#define VKSIFT_EXT_DESCRIBE_GIVEN 1u
  VKSIFT_EXPORT void vksift_ext_describeKeypoints(vksift_Instance instance, const uint8_t *image_data, uint32_t image_width, uint32_t image_height,
                                                  const vksift_ext_Keypoint *kps, uint32_t nb_kps, uint32_t gpu_buffer_id, uint32_t mode);
  VKSIFT_EXPORT void vksift_ext_describeKeypointsBatch(vksift_Instance instance, const uint8_t *const *images, uint32_t count, uint32_t image_width,
                                                       uint32_t image_height, const vksift_ext_Keypoint *kps, const uint32_t *nb_kps,
                                                       uint32_t first_gpu_buffer_id, uint32_t mode);
  VKSIFT_EXPORT uint32_t vksift_ext_getPlacedKeypointsNumber(vksift_Instance instance, uint32_t gpu_buffer_id);

  /* Deferred submission of vksift_detectFeatures (no counterpart in the reference, no change of its contract): consecutive plain
   * detect calls into consecutive SIFT buffers, with nothing asked in between, are staged and launched as ONE batched detection by
   * the first call that needs a result — any other entry point — or when 128 images (VKSIFT_DEFER_MAX) are staged, or 16 (VKSIFT_DEFER_CHUNK)
   * while the GPU has no detection to work on. The first detect
   * call after another entry point is launched at once unless the caller's previous run of detect calls held two or more, so
   * detect + read and the two-buffer ping-pong keep their latency. VKSIFT_DEFER=0 launches every call at once. Results are
   * identical either way; the scale-space accessors (vksift_downloadScaleSpaceImage, vksift_downloadDoGImage) show the last plain
   * detection either way, and image 0 of the batch after a vksift_ext_detectFeaturesBatch* call. These counters say what the
   * instance did: batches launched from staged images, and images in them. */
  VKSIFT_EXPORT void vksift_ext_getDeferredStats(vksift_Instance instance, uint64_t *nb_batches, uint64_t *nb_images);

  /* Stage timings (milliseconds, HIP events on the instance stream) of the last detect call.
   * Enabled with vksift_ext_setProfiling(instance, true); disabled by default. Blocking. */
  typedef struct
  {
    float upload_ms;      /* host->device image copy */
    float pyramid_ms;     /* input blit + all blur/DoG + down-sample launches */
    float extrema_ms;     /* detect + scan + emit */
    float orientation_ms;
    float descriptor_ms;
    float total_ms;
    uint32_t nb_blur_launches;
    uint64_t pyramid_algorithmic_bytes; /* SURVEY.md §8(d) definition, whole batch */
    float scan_ms;                      /* the streaming extrema scan of octave 0 alone (mask clear + the kernel that reads the S+3 planes) */
    uint64_t scan_algorithmic_bytes;    /* 4*(S+2) B per octave-0 pixel, whole batch */
    float pyramid_all_ms;               /* the scale-space construction of EVERY octave: first launch of octave 0 to the last blur launch of the
                                         * coarsest octave, on the stream they run on (pyramid_ms: octave 0 alone) */
    uint32_t nb_blur_launches_all;      /* launches inside that interval */
  } vksift_ext_DetectTimings;
  /* The struct grew twice (scan_ms, scan_algorithmic_bytes; pyramid_all_ms, nb_blur_launches_all) and may grow again at its end. The two getters without a size
   * argument therefore write only the first VKSIFT_EXT_DETECT_TIMINGS_V1_BYTES bytes — the struct of the first release, so a
   * client compiled against that header is never written past its storage; the ...Sized forms write min(out_bytes, sizeof)
   * bytes of the current struct (pass sizeof(vksift_ext_DetectTimings) of the header you compiled against). */
#define VKSIFT_EXT_DETECT_TIMINGS_V1_BYTES 40u
  VKSIFT_EXPORT void vksift_ext_setProfiling(vksift_Instance instance, bool enabled);
  VKSIFT_EXPORT void vksift_ext_getDetectTimings(vksift_Instance instance, vksift_ext_DetectTimings *out);
  VKSIFT_EXPORT void vksift_ext_getDetectTimingsSized(vksift_Instance instance, vksift_ext_DetectTimings *out, size_t out_bytes);
  /* Sums over all detect calls since profiling was enabled (or since the last reset); nb_blur_launches and
   * pyramid_algorithmic_bytes are summed too. Blocking. */
  VKSIFT_EXPORT void vksift_ext_getAccumulatedDetectTimings(vksift_Instance instance, vksift_ext_DetectTimings *sum, uint32_t *nb_calls, bool reset);
  VKSIFT_EXPORT void vksift_ext_getAccumulatedDetectTimingsSized(vksift_Instance instance, vksift_ext_DetectTimings *sum, size_t sum_bytes, uint32_t *nb_calls,
                                                                  bool reset);
  /* Clients compiled against THIS header get every field: the unsized names expand to the ...Sized forms with the size of the
   * struct they were compiled with. The exported symbols of the same names keep the 40-byte behaviour for binaries built against
   * the first release (which pass a 40-byte struct). */
#ifndef VKSIFT_BUILD
#define vksift_ext_getDetectTimings(instance, out) vksift_ext_getDetectTimingsSized((instance), (out), sizeof(vksift_ext_DetectTimings))
#define vksift_ext_getAccumulatedDetectTimings(instance, sum, nb_calls, reset) \
  vksift_ext_getAccumulatedDetectTimingsSized((instance), (sum), sizeof(vksift_ext_DetectTimings), (nb_calls), (reset))
#endif
  /* Where the scale-space was put: batch instances time a whole-batch blur launch on candidate memory ranges
   * when they allocate their scale-space buffers and keep the fastest. gbps[0 .. n): the rate of that launch (8 B per texel) on every
   * candidate in allocation order, chosen[0 .. 1]: the indices in use (chosen[1] = chosen[0] unless the instance holds two buffers: VKSIFT_PYR_PINGPONG=2). Returns n — 0 when the
   * buffers were allocated plainly (single-image instances, VKSIFT_PYR_PLACEMENT=0). */
  VKSIFT_EXPORT uint32_t vksift_ext_getScaleSpacePlacement(vksift_Instance instance, float gbps[8], uint32_t chosen[2]);

  /* Page-locked result buffers. vksift_downloadFeatures / vksift_ext_downloadMatchesBatch copy device -> pinned staging -> the caller's
   * (pageable) array: the second hop is a host memcpy at ~10 GB/s, 15 ms per 512 VGA frames' features — more than the bus takes. A
   * destination that is page-locked — registered here (hipHostRegister underneath), or any memory hipHostMalloc returned — receives the
   * records of a batched detection / matching by DMA straight from device memory: no staging, no host copy. Register once, reuse the
   * buffer. Both return VKSIFT_SUCCESS or VKSIFT_VULKAN_ERROR. For callers that fetch while the GPU is otherwise idle: with a detection
   * queued behind, every such transfer waits in the copy engine's ring (77 us each on MI355X against 7.5 us for the staged path, which
   * moves the whole detection in a few large pieces). */
  VKSIFT_EXPORT vksift_Result vksift_ext_pinHostMemory(void *ptr, size_t bytes);
  VKSIFT_EXPORT vksift_Result vksift_ext_unpinHostMemory(void *ptr);

  /* Time (ms) of the last matching pipeline (gather + 2-NN kernel), HIP events; needs profiling on.
   * This getter and every other stage getter (vksift_ext_getVerifyTime ... vksift_ext_getTracksTime, vksift_ext_getRootSiftTime) waits for the
   * instance's streams before it reads its events: if that wait fails the error callback fires with VKSIFT_VULKAN_ERROR and the getter returns -1.
   * A stage whose interval could not be closed (the end event's record failed: the stage itself reports VKSIFT_VULKAN_ERROR) has no time: -1. */
  VKSIFT_EXPORT float vksift_ext_getMatchTime(vksift_Instance instance);

  /* Copy the descriptors of a SIFT buffer, in download order, as dense 128-byte rows into caller
   * provided DEVICE memory (>= vksift_getFeaturesNumber()*128 bytes, 16-byte aligned). Blocking.
   * Returns the number of rows written. Used to feed the RCCL all-gather of the sharded matcher. */
  VKSIFT_EXPORT uint32_t vksift_ext_exportDescriptorsDevice(vksift_Instance instance, uint32_t gpu_buffer_id, uint8_t *d_descriptors);

  /* ---------------------------------------------------------------------------------------------------------------
   * Sharded 2-NN matching over the GPUs of one node. One process per GPU. The query rows of A are sharded
   * by the caller (any split); the reference set B is sharded in equal blocks of nb_shard = ceil(nb_total / world) rows
   * (rank r holds rows [r*nb_shard, ...); rows past nb_total are padding) and all-gathered ONCE inside the call: an RCCL
   * all-gather of uint8 rows over xGMI, issued first and overlapped with the norm pre-pass of the local A rows. Every
   * rank then scans all of B in index order, so the records are bit-identical to a single-GPU vksift_matchFeatures for
   * every world size. RCCL is loaded on first use (dlopen).
   *   rank 0: vksift_ext_shardGetUniqueId(id), then send the 128 bytes to the other ranks by any host channel
   *   all   : vksift_ext_shardGroupCreate(&group, device, world, rank, id)      (collective: ncclCommInitRank)
   *   all   : vksift_ext_matchSharded(...)                                       (collective, asynchronous on the group's stream)
   *   all   : vksift_ext_shardGroupSynchronize(group, &ms)
   * d_a_rows / d_b_shard / d_matches are DEVICE pointers (dense 128-byte rows; na records of 20 bytes = vksift_Match_2NN with
   * idx_a = a_index_base + row). vksift_ext_exportDescriptorsDevice() produces such rows from a SIFT buffer. */
#define VKSIFT_EXT_SHARD_ID_BYTES 128
  typedef struct vksift_ext_ShardGroup_T *vksift_ext_ShardGroup;
  VKSIFT_EXPORT vksift_Result vksift_ext_shardGetUniqueId(uint8_t id[VKSIFT_EXT_SHARD_ID_BYTES]);
  VKSIFT_EXPORT vksift_Result vksift_ext_shardGroupCreate(vksift_ext_ShardGroup *group_ptr, int gpu_device_index, uint32_t world, uint32_t rank,
                                                          const uint8_t id[VKSIFT_EXT_SHARD_ID_BYTES]);
  /* The same group over the APPLICATION's transport instead of RCCL (an MPI job, a host-staged exchange, a test harness): the
   * callback stands in for ncclAllGather and has its contract — every rank contributes bytes_per_rank bytes at d_send, rank r's
   * block lands at d_recv + r * bytes_per_rank on every rank (d_send may already BE this rank's slot of d_recv), ordered on
   * hip_stream (a hipStream_t): it must see everything queued on hip_stream before the call, and work queued on hip_stream after
   * it returns must see the gathered data (a blocking implementation synchronises hip_stream first). Returns 0 on success. Not
   * collective itself; RCCL is neither loaded nor needed. */
  typedef int (*vksift_ext_AllGatherFn)(void *user, const void *d_send, void *d_recv, size_t bytes_per_rank, uint32_t rank, uint32_t world,
                                        void *hip_stream);
  VKSIFT_EXPORT vksift_Result vksift_ext_shardGroupCreateWithTransport(vksift_ext_ShardGroup *group_ptr, int gpu_device_index, uint32_t world, uint32_t rank,
                                                                       vksift_ext_AllGatherFn all_gather, void *user);
  /* The block layout of the reference set that vksift_ext_matchSharded all-gathers: block_rows = ceil(n_total / world) (= nb_shard),
   * rank `rank` holds rows [first_row, first_row + nb_rows) of B (nb_rows <= block_rows; the rest of its block is padding). Pure
   * arithmetic (no GPU needed); callers that shard the query rows the same way use first_row as a_index_base. */
  /* What the group runs on: (world, rank) as created, and ncclCommCount / ncclCommUserRank of its RCCL communicator — 0 / 0 for a group
   * over the application's transport. A creation whose communicator disagrees with (world, rank) fails; a caller that prints
   * rccl_ranks proves how many ranks RCCL itself saw (bench.py does). */
  VKSIFT_EXPORT void vksift_ext_shardGroupInfo(vksift_ext_ShardGroup group, uint32_t *world, uint32_t *rank, uint32_t *rccl_ranks, uint32_t *rccl_rank);
  VKSIFT_EXPORT void vksift_ext_shardGroupLayout(uint32_t n_total, uint32_t world, uint32_t rank, uint32_t *block_rows, uint32_t *first_row,
                                                 uint32_t *nb_rows);
  VKSIFT_EXPORT void vksift_ext_shardGroupDestroy(vksift_ext_ShardGroup *group_ptr);
  /* Local, not collective: reserves the device scratch for matchings of up to max_na local query rows against up to max_nb_total
   * reference rows. A vksift_ext_matchSharded within the reservation allocates nothing, so it cannot fail for resources before its
   * collective (a rank that cannot allocate the receive buffer inside matchSharded has to abort the communicator: see there). */
  VKSIFT_EXPORT vksift_Result vksift_ext_shardGroupReserve(vksift_ext_ShardGroup group, uint32_t max_na, uint32_t max_nb_total);
  /* Collective. Error discipline: nb_shard / nb_total (identical on every rank) are validated before anything is queued; a rank with
   * a local failure (NULL local pointer, no scratch memory) still enters the all-gather and then returns its error, so its peers are
   * not left blocked; only a missing receive buffer aborts the communicator (group unusable afterwards). */
  VKSIFT_EXPORT vksift_Result vksift_ext_matchSharded(vksift_ext_ShardGroup group, const uint8_t *d_a_rows, uint32_t na, uint32_t a_index_base,
                                                      const uint8_t *d_b_shard, uint32_t nb_shard, uint32_t nb_total, uint8_t *d_matches);
  VKSIFT_EXPORT vksift_Result vksift_ext_shardGroupSynchronize(vksift_ext_ShardGroup group, float *last_match_ms);

  /* Deterministic synthetic test image: 128 + sum of Gaussian blobs + uniform noise,
   * splitmix64-seeded, clamped to [0,255]. nb_blobs == 0 picks the density used by the benchmarks. */
  VKSIFT_EXPORT void vksift_ext_genSyntheticImage(uint64_t seed, uint32_t width, uint32_t height, uint32_t nb_blobs, uint8_t *out);
  /* Further deterministic image families (the parity tests' second and third opinion on what an image looks like):
   * BLOBS = vksift_ext_genSyntheticImage with the benchmark density; EDGES = flat rotated rectangles and checker patches over a
   * ramp (long step edges, corners, junctions, shapes cut by the border); FRACTAL = 1/f value noise (texture at every scale). */
#define VKSIFT_EXT_SYNTH_BLOBS 0u
#define VKSIFT_EXT_SYNTH_EDGES 1u
#define VKSIFT_EXT_SYNTH_FRACTAL 2u
  VKSIFT_EXPORT void vksift_ext_genSyntheticImageFamily(uint64_t seed, uint32_t width, uint32_t height, uint32_t family, uint8_t *out);
  /* Deterministic SIFT-like descriptor rows: min(255, trunc(512*|g|/||g||)), g ~ N(0,1)^128. */
  VKSIFT_EXPORT void vksift_ext_genSyntheticDescriptors(uint64_t seed, uint32_t rows, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif /* VKSIFT_EXT_H */
