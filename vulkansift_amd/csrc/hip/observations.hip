// observations.hip — the observation table of the tracks vksift_hip_build_tracks left: the selected tracks as CSR offsets plus one 16-byte record
// {gpu_buffer_id, row, x, y} per member (vksift_hip_track_observations; no counterpart in the reference, whose callers download the per-feature words and
// every feature record and group them with a host sort). DESIGN.md, "Track observations", holds the argument; the header (include/vksift_hip.h) the contract.
//
// The members of a track are scattered over the buffers; what brings them together is a stable sort of the nodes by their track's new number. Elements
// are the slots of tracks.hip's per-node launches (blocks of 256 rows per buffer rank), so element order is the order (gpu_buffer_id, row) and a stable
// sort leaves the members of a track in that order. A launch sequence on one stream; every phase that reads another phase's plain stores is a launch
// of its own:
//   k_obs_select   one lane per track record: the selection test; per block the selected tracks, their lengths and the two rejection counts
//   k_obs_totals   exclusive scan of the first two, the four statistics and offsets[nb_tracks] (one workgroup)
//   k_obs_number   block scan + block offset = new number and first observation: offsets, track_ids, and the map old number -> new number or none
//   k_obs_xy       {x, y} of every stored row, by node; a buffer's layout is resolved once per workgroup in LDS (records.h)
//   k_obs_keys     element -> {key, node}: the new number of the node's track, OBS_NONE for everything else (it sorts to the tail)
//   per 8-bit digit, low to high (LSD radix sort; the number of passes is the host's, from the bound on the track count):
//     k_obs_hist     per block of OBS_TILE elements the 256 digit counts, into a digit-major table
//     k_obs_scan     exclusive scan of the table (one workgroup)
//     k_obs_scatter  stable scatter: match groups per wave by ballot, the waves' counts per digit through LDS, the block's base from the table
//   k_obs_expand   position p < nb_observations of the sorted list -> {buf_tab id, row, xy[node]}
// No atomics on global memory, no lane waits for another workgroup, every grid and loop is bounded by the launcher's arguments (counts read on the
// device are clamped to them), and every output depends on the inputs alone.
#include "vksift_hip.h"
#include "hip/records.h"
#include "wave.h"

#include <hip/hip_runtime.h>

#define OBS_THREADS 256u
#define OBS_ITEMS 8u                          /* rounds of 256 elements a sort block serves */
#define OBS_TILE (OBS_THREADS * OBS_ITEMS)    /* elements per sort block: the digit table is an eighth of the element count */
#define OBS_NONE 0xFFFFFFFFu                  /* no node / no track / the key of an element that is no member of a selected track */

namespace
{

// the stored rows of the buffer of rank `rank` (tracks.hip's rule: the count on the device, clamped)
__device__ __forceinline__ uint32_t obs_buf_rows(const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t rank, uint32_t max_rows)
{
  const uint32_t n = rows_dev[buf_tab[2u * rank + 1u]];
  return n < max_rows ? n : max_rows;
}

// the tracks there are: the count vksift_hip_build_tracks left on the device, clamped to the host's bound
__device__ __forceinline__ uint32_t obs_tracks(const uint32_t *track_stats, uint32_t tracks_bound)
{
  const uint32_t n = track_stats[0];
  return n < tracks_bound ? n : tracks_bound;
}

// 0: selected, 1: fails the length test, 2: passes it and is dropped as conflicting
__device__ __forceinline__ uint32_t obs_verdict(uint32_t len, uint32_t nbuf, uint32_t min_length, uint32_t max_length, uint32_t conflicts)
{
  if (len < min_length || (max_length != 0u && len > max_length))
    return 1u;
  return (conflicts != 0u && len != nbuf) ? 2u : 0u;
}

// sum over the workgroup of 256, in every thread (part: LDS of the caller; a barrier before it is used again)
__device__ __forceinline__ uint32_t block_sum_256(uint32_t v, uint32_t (&part)[4])
{
  const uint32_t w = wave_sum_u32(v);
  if ((threadIdx.x & 63u) == 0u)
    part[threadIdx.x >> 6] = w;
  __syncthreads();
  const uint32_t t = part[0] + part[1] + part[2] + part[3];
  __syncthreads();
  return t;
}

// bsum: four arrays of gridDim.x words — selected tracks, their lengths, rejected by length, rejected as conflicting
__global__ __launch_bounds__(OBS_THREADS) void k_obs_select(const uint32_t *tracks, const uint32_t *track_stats, uint32_t tracks_bound, uint32_t min_length,
                                                            uint32_t max_length, uint32_t conflicts, uint32_t *bsum)
{
  __shared__ uint32_t part[4];
  const uint32_t t = blockIdx.x * OBS_THREADS + threadIdx.x;
  uint32_t verdict = 3u, len = 0;
  if (t < obs_tracks(track_stats, tracks_bound))
  {
    len = tracks[4u * (size_t)t + 2u];
    verdict = obs_verdict(len, tracks[4u * (size_t)t + 3u], min_length, max_length, conflicts);
  }
  const uint32_t sel = block_sum_256(verdict == 0u, part), members = block_sum_256(verdict == 0u ? len : 0u, part);
  const uint32_t rej_len = block_sum_256(verdict == 1u, part), rej_conf = block_sum_256(verdict == 2u, part);
  if (threadIdx.x == 0)
  {
    bsum[blockIdx.x] = sel;
    bsum[gridDim.x + blockIdx.x] = members;
    bsum[2u * gridDim.x + blockIdx.x] = rej_len;
    bsum[3u * gridDim.x + blockIdx.x] = rej_conf;
  }
}

// a[0 .. n) becomes its exclusive prefix sum; returns the total in every thread. One workgroup of 1024; wsum: 17 words of LDS.
__device__ __forceinline__ uint32_t scan_excl_1024(uint32_t *a, uint32_t n, uint32_t (&wsum)[17])
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += 1024u)
  {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n ? a[i] : 0u;
    const uint32_t incl = wave_scan_incl_u32(v, lane);
    if (lane == 63)
      wsum[wave] = incl;
    __syncthreads();
    if (wave == 0)
    {
      const uint32_t t = lane < 16 ? wsum[lane] : 0u;
      const uint32_t ti = wave_scan_incl_u32(t, lane);
      if (lane < 16)
        wsum[lane] = ti - t;
      if (lane == 15)
        wsum[16] = ti;
    }
    __syncthreads();
    if (i < n)
      a[i] = carry + wsum[wave] + incl - v;
    carry += wsum[16];
    __syncthreads();
  }
  return carry;
}

// sum of a[0 .. n) in every thread of a workgroup of 1024 (wsum as above)
__device__ __forceinline__ uint32_t sum_1024(const uint32_t *a, uint32_t n, uint32_t (&wsum)[17])
{
  uint32_t v = 0;
  for (uint32_t i = threadIdx.x; i < n; i += 1024u)
    v += a[i];
  v = wave_sum_u32(v);
  if ((threadIdx.x & 63u) == 0u)
    wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
  for (int w = 0; w < 16; w++)
    t += wsum[w];
  __syncthreads();
  return t;
}

// the select launch's four arrays: the first two become exclusive prefix sums; stats = {selected tracks, observations, rejected by length, rejected as
// conflicting}; offsets[selected tracks] = observations (offsets[0] = 0 with none)
__global__ __launch_bounds__(1024) void k_obs_totals(uint32_t *bsum, uint32_t nblocks, uint32_t *stats, uint32_t *offsets)
{
  __shared__ uint32_t wsum[17];
  const uint32_t sel = scan_excl_1024(bsum, nblocks, wsum), members = scan_excl_1024(bsum + nblocks, nblocks, wsum);
  const uint32_t rej_len = sum_1024(bsum + 2u * (size_t)nblocks, nblocks, wsum), rej_conf = sum_1024(bsum + 3u * (size_t)nblocks, nblocks, wsum);
  if (threadIdx.x == 0)
  {
    stats[0] = sel, stats[1] = members, stats[2] = rej_len, stats[3] = rej_conf;
    offsets[sel] = members;
  }
}

// the digit table of one sort pass becomes its exclusive prefix sum
__global__ __launch_bounds__(1024) void k_obs_scan(uint32_t *table, uint32_t n)
{
  __shared__ uint32_t wsum[17];
  (void)scan_excl_1024(table, n, wsum);
}

__global__ __launch_bounds__(OBS_THREADS) void k_obs_number(const uint32_t *tracks, const uint32_t *track_stats, uint32_t tracks_bound, uint32_t min_length,
                                                            uint32_t max_length, uint32_t conflicts, const uint32_t *bsum, uint32_t *offsets, uint32_t *track_ids,
                                                            uint32_t *map)
{
  __shared__ uint32_t wcnt[4], wlen[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t t = blockIdx.x * OBS_THREADS + threadIdx.x;
  const bool there = t < obs_tracks(track_stats, tracks_bound);
  uint32_t len = 0;
  bool sel = false;
  if (there)
  {
    len = tracks[4u * (size_t)t + 2u];
    sel = obs_verdict(len, tracks[4u * (size_t)t + 3u], min_length, max_length, conflicts) == 0u;
  }
  len = sel ? len : 0u;
  const unsigned long long bal = __ballot(sel);
  const uint32_t incl = wave_scan_incl_u32(len, lane);
  if (lane == 63)
    wcnt[wave] = (uint32_t)__popcll(bal), wlen[wave] = incl;
  __syncthreads();
  uint32_t m = bsum[blockIdx.x] + ballot_rank(bal, lane), first = bsum[gridDim.x + blockIdx.x] + incl - len;
  for (int w = 0; w < wave; w++)
    m += wcnt[w], first += wlen[w];
  if (sel)
    offsets[m] = first, track_ids[m] = t;
  if (there)
    map[t] = sel ? m : OBS_NONE;
}

// block b serves rows [256 (b % bpb), ...) of the buffer of rank b / bpb (tracks.hip's per-node launches). A row the tracks know that the buffer's
// layout does not hold (the buffer was refilled since the matching) gets zeros, so that every word the later launches read is written.
__global__ __launch_bounds__(OBS_THREADS) void k_obs_xy(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *found_base, uint32_t found_buf_stride,
                                                        const uint32_t *buf_tab, const uint32_t *rows_dev, const uint32_t *rank_layouts, const uint32_t *layouts,
                                                        uint32_t bpb, uint32_t node_stride, uint32_t max_rows, float2 *xy)
{
  __shared__ SideLayout L[1];
  __shared__ uint32_t slot[4];
  const uint32_t rank = blockIdx.x / bpb, row = (blockIdx.x % bpb) * OBS_THREADS + threadIdx.x;
  if (threadIdx.x == 0)
    slot[0] = buf_tab[2u * rank], slot[1] = 0u, slot[2] = rank_layouts[rank], slot[3] = 0u;
  __syncthreads();
  layout_decode(L, slot, 0u, layouts, found_base, found_buf_stride);
  if (row >= obs_buf_rows(buf_tab, rows_dev, rank, max_rows))
    return;
  float2 v = float2{0.f, 0.f};
  if (row < L[0].total)
  {
    const float *f = (const float *)(feats_base + (size_t)L[0].buf * buf_stride + (size_t)section_row(L[0].cnt, L[0].off, row) * VKSIFT_RECORD_BYTES);
    v = float2{f[0], f[1]};
  }
  xy[(size_t)rank * node_stride + row] = v;
}

// element e < nelems: rank e / (256 bpb), row e % (256 bpb). Elements at and beyond nelems (the last sort block's padding) are written too.
__global__ __launch_bounds__(OBS_THREADS) void k_obs_keys(const uint32_t *node_words, const uint32_t *map, const uint32_t *track_stats, uint32_t tracks_bound,
                                                          const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t bpb, uint32_t node_stride, uint32_t max_rows,
                                                          uint32_t nelems, uint32_t *keys, uint32_t *vals)
{
  const uint32_t e = blockIdx.x * OBS_THREADS + threadIdx.x;
  uint32_t key = OBS_NONE, node = OBS_NONE;
  if (e < nelems)
  {
    const uint32_t rank = e / (bpb * OBS_THREADS), row = e % (bpb * OBS_THREADS);
    if (row < obs_buf_rows(buf_tab, rows_dev, rank, max_rows))
    {
      node = rank * node_stride + row;
      const uint32_t w = node_words[node];
      if (w < obs_tracks(track_stats, tracks_bound))
        key = map[w];
    }
  }
  keys[e] = key, vals[e] = node;
}

// table[d * gridDim.x + block] = the elements of the block whose digit is d
__global__ __launch_bounds__(OBS_THREADS) void k_obs_hist(const uint32_t *keys, uint32_t shift, uint32_t *table)
{
  __shared__ uint32_t hist[256];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t *k = keys + (size_t)blockIdx.x * OBS_TILE;
  for (uint32_t r = 0; r < OBS_ITEMS; r++)
    atomicAdd(&hist[(k[r * OBS_THREADS + threadIdx.x] >> shift) & 255u], 1u); // LDS
  __syncthreads();
  table[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = hist[threadIdx.x];
}

// The block's elements go, in element order, behind the elements of the blocks in front of it that share their digit: rounds of 256 in order, inside a
// round the waves in order, inside a wave the lanes in order.
__global__ __launch_bounds__(OBS_THREADS) void k_obs_scatter(const uint32_t *keys, const uint32_t *vals, uint32_t shift, const uint32_t *table, uint32_t *keys_out,
                                                             uint32_t *vals_out)
{
  __shared__ uint32_t base[256], wcnt[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  base[threadIdx.x] = table[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
  for (int w = 0; w < 4; w++)
    wcnt[w][threadIdx.x] = 0;
  __syncthreads();
  const size_t first = (size_t)blockIdx.x * OBS_TILE;
  for (uint32_t r = 0; r < OBS_ITEMS; r++)
  {
    const uint32_t key = keys[first + r * OBS_THREADS + threadIdx.x], val = vals[first + r * OBS_THREADS + threadIdx.x];
    const uint32_t d = (key >> shift) & 255u;
    // the lanes of the wave with this lane's digit
    unsigned long long same = ~0ull;
#pragma unroll
    for (uint32_t b = 0; b < 8u; b++)
    {
      const unsigned long long bal = __ballot((d >> b) & 1u);
      same &= ((d >> b) & 1u) ? bal : ~bal;
    }
    const uint32_t rank = ballot_rank(same, lane);
    if (rank == 0u)
      wcnt[wave][d] = (uint32_t)__popcll(same); // (one lane per digit and wave)
    __syncthreads();
    uint32_t pos = base[d] + rank;
    for (int w = 0; w < wave; w++)
      pos += wcnt[w][d];
    keys_out[pos] = key, vals_out[pos] = val;
    __syncthreads();
    // thread d owns digit d: the round's elements are placed, the counts return to zero
    base[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
    for (int w = 0; w < 4; w++)
      wcnt[w][threadIdx.x] = 0;
    __syncthreads();
  }
}

__global__ __launch_bounds__(OBS_THREADS) void k_obs_expand(const uint32_t *vals, const float2 *xy, const uint32_t *stats, uint32_t obs_bound, const uint32_t *buf_tab,
                                                            uint32_t node_stride, uint4 *obs)
{
  const uint32_t p = blockIdx.x * OBS_THREADS + threadIdx.x;
  const uint32_t n = stats[1] < obs_bound ? stats[1] : obs_bound;
  if (p >= n)
    return;
  const uint32_t node = vals[p];
  if (node == OBS_NONE) // (never: the first nb_observations elements of the sorted list are members)
    return;
  const float2 v = xy[node];
  obs[p] = uint4{buf_tab[2u * (node / node_stride)], node % node_stride, __float_as_uint(v.x), __float_as_uint(v.y)};
}

// what the launcher and the scratch size share
struct ObsDims
{
  uint64_t nodes, tracks_bound, obs_bound, bpb, nelems, sort_blocks, select_blocks;
};

inline ObsDims obs_dims(uint32_t nbufs, uint32_t node_stride, uint32_t max_rows)
{
  ObsDims d;
  d.nodes = (uint64_t)nbufs * node_stride;
  d.obs_bound = (uint64_t)nbufs * max_rows;
  d.tracks_bound = d.obs_bound / 2u;
  d.bpb = ((uint64_t)max_rows + OBS_THREADS - 1u) / OBS_THREADS;
  d.nelems = (uint64_t)nbufs * d.bpb * OBS_THREADS;
  d.sort_blocks = (d.nelems + OBS_TILE - 1u) / OBS_TILE;
  d.select_blocks = d.tracks_bound ? (d.tracks_bound + OBS_THREADS - 1u) / OBS_THREADS : 1u;
  return d;
}

} // namespace

extern "C" size_t vksift_hip_observations_scratch_u32(uint32_t nbufs, uint32_t node_stride, uint32_t max_rows)
{
  const ObsDims d = obs_dims(nbufs, node_stride, max_rows);
  // xy by node, two {key, node} lists of whole sort blocks, the digit table, the map, the select launch's four arrays, and two
  return (size_t)(2u * d.nodes + 4u * d.sort_blocks * OBS_TILE + 256u * d.sort_blocks + d.tracks_bound + 4u * d.select_blocks + 2u);
}

extern "C" int vksift_hip_track_observations(const uint32_t *node_words, const uint8_t *tracks, const uint32_t *track_stats, const uint32_t *buf_tab, uint32_t nbufs,
                                             const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, const uint8_t *feats_base, uint64_t buf_stride,
                                             const uint32_t *found_base, uint32_t found_buf_stride, const uint32_t *rank_layouts, const uint32_t *layouts,
                                             uint32_t min_length, uint32_t max_length, uint32_t conflicts, uint32_t *offsets, uint32_t *track_ids, uint64_t tracks_cap,
                                             uint8_t *observations, uint64_t obs_cap, uint32_t *stats, uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s)
{
  const ObsDims d = obs_dims(nbufs, node_stride, max_rows);
  if (nbufs == 0 || max_rows == 0 || max_rows > node_stride || d.nodes >= 0xFFFFFFFFull || d.sort_blocks * OBS_TILE > 0x7FFFFFFFull || min_length < 2u ||
      (max_length != 0u && max_length < min_length) || conflicts > 1u || ((uintptr_t)tracks & 3u) || ((uintptr_t)feats_base & 3u) || (buf_stride & 3u) ||
      ((uintptr_t)observations & 15u) || ((uintptr_t)scratch & 7u) || tracks_cap < d.tracks_bound || obs_cap < d.obs_bound ||
      scratch_u32 < vksift_hip_observations_scratch_u32(nbufs, node_stride, max_rows))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)s;
  const uint32_t bpb = (uint32_t)d.bpb, nelems = (uint32_t)d.nelems, sort_blocks = (uint32_t)d.sort_blocks, select_blocks = (uint32_t)d.select_blocks;
  const uint32_t tracks_bound = (uint32_t)d.tracks_bound, obs_bound = (uint32_t)d.obs_bound;
  const size_t padded = (size_t)sort_blocks * OBS_TILE;
  float2 *xy = (float2 *)scratch;
  uint32_t *keys[2], *vals[2];
  keys[0] = scratch + 2u * d.nodes, vals[0] = keys[0] + padded, keys[1] = vals[0] + padded, vals[1] = keys[1] + padded;
  uint32_t *table = vals[1] + padded, *map = table + 256u * (size_t)sort_blocks, *bsum = map + tracks_bound;
  const uint32_t *trk = (const uint32_t *)tracks;

  k_obs_select<<<select_blocks, OBS_THREADS, 0, st>>>(trk, track_stats, tracks_bound, min_length, max_length, conflicts, bsum);
  k_obs_totals<<<1, 1024, 0, st>>>(bsum, select_blocks, stats, offsets);
  k_obs_number<<<select_blocks, OBS_THREADS, 0, st>>>(trk, track_stats, tracks_bound, min_length, max_length, conflicts, bsum, offsets, track_ids, map);
  k_obs_xy<<<nbufs * bpb, OBS_THREADS, 0, st>>>(feats_base, buf_stride, found_base, found_buf_stride, buf_tab, rows_dev, rank_layouts, layouts, bpb, node_stride,
                                                max_rows, xy);
  k_obs_keys<<<sort_blocks * OBS_ITEMS, OBS_THREADS, 0, st>>>(node_words, map, track_stats, tracks_bound, buf_tab, rows_dev, bpb, node_stride, max_rows, nelems, keys[0],
                                                              vals[0]);
  // a key is below tracks_bound or OBS_NONE, whose digits are all 255: `passes` digits order them as long as tracks_bound < 256^passes
  uint32_t passes = 1;
  while (passes < 4u && (tracks_bound >> (8u * passes)) != 0u)
    passes++;
  uint32_t cur = 0;
  for (uint32_t p = 0; p < passes; p++, cur ^= 1u)
  {
    k_obs_hist<<<sort_blocks, OBS_THREADS, 0, st>>>(keys[cur], 8u * p, table);
    k_obs_scan<<<1, 1024, 0, st>>>(table, 256u * sort_blocks);
    k_obs_scatter<<<sort_blocks, OBS_THREADS, 0, st>>>(keys[cur], vals[cur], 8u * p, table, keys[cur ^ 1u], vals[cur ^ 1u]);
  }
  k_obs_expand<<<(obs_bound + OBS_THREADS - 1u) / OBS_THREADS, OBS_THREADS, 0, st>>>(vals[cur], xy, stats, obs_bound, buf_tab, node_stride, (uint4 *)observations);
  return (int)hipGetLastError();
}
