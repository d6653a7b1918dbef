// track_edges.hip — feature tracks across matching calls: an edge store that outlives a matching (vksift_hip_append_track_edges) and the tracks of the
// graph it holds (vksift_hip_build_tracks_from_edges). No counterpart in the reference, whose callers keep every pair's matches on the host. DESIGN.md,
// "Tracks across matching calls", holds the argument; the header (include/vksift_hip.h) the contract; tests/np_track_edges.py restates both.
//
// Append is an ordered compaction over (slot, block of 256 records), three launches on one stream, each reading the plain stores of the one before:
//   k_edges_count  per (slot, block) the records that are edges, by the rule of k_tracks_hook (tracks.h: pair_edge)
//   k_edges_scan   one workgroup: the counts become offsets that start at the store's count and stop at its capacity; the statistics; the row table
//   k_edges_write  every edge to offset + its rank among the block's edges: slot ascending, record ascending
// No atomics, no lane waits for another workgroup, every output depends on the inputs alone.
// Build: tracks.hip's init launch, k_edges_hook (one lane per stored edge: both buffers to ranks, both rows against the row table, then the union of
// tracks.h, whose visibility argument is the one of DESIGN.md, "Tracks": agent-scope atomics on the parent words, nothing else), tracks.hip's tail.
#include "vksift_hip.h"
#include "tracks.h"

#include <hip/hip_runtime.h>

#define EDGE_UNSET 0xFFFFFFFFu /* a word of the row table no call has recorded a count in */

__global__ __launch_bounds__(TRK_THREADS) void k_edges_count(PairEdges in, uint32_t *cnt)
{
  uint32_t *out = cnt + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (pair_block_idle(in))
  {
    if (threadIdx.x == 0)
      *out = 0;
    return;
  }
  uint32_t ra, ia, rb, ib;
  const uint32_t n = (uint32_t)__syncthreads_count(pair_edge(in, ra, ia, rb, ib));
  if (threadIdx.x == 0)
    *out = n;
}

// cnt[0 .. nblocks) becomes min(start + its exclusive prefix sum, max_edges) with start = min(stats[0], max_edges), the store's count. stats: {edges held,
// edges dropped, calls, changed buffers}. The row table: the count of every buffer of the call that has none yet; a buffer whose count differs from the one
// recorded adds 1 to the changed buffers and keeps its word. One workgroup of 1024.
__global__ __launch_bounds__(1024) void k_edges_scan(uint32_t *cnt, uint32_t nblocks, const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t *row_table,
                                                     uint32_t nb_buffers, uint32_t max_edges, uint32_t *stats)
{
  __shared__ uint32_t wsum[17], wchg[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t held = stats[0], dropped = stats[1], calls = stats[2], changed_before = stats[3]; // (written by lane 0 behind the barriers below)
  const u64 start = held < max_edges ? held : max_edges;
  u64 carry = 0;
  for (uint32_t base = 0; base < nblocks; base += 1024u)
  {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nblocks ? cnt[i] : 0u;
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
    if (i < nblocks)
    {
      const u64 at = start + carry + wsum[wave] + incl - v;
      cnt[i] = at < max_edges ? (uint32_t)at : max_edges;
    }
    carry += wsum[16];
    __syncthreads();
  }
  uint32_t changed = 0;
  for (uint32_t r = threadIdx.x; r < nbufs; r += 1024u)
  {
    const uint32_t id = buf_tab[2u * r], raw = rows_dev[buf_tab[2u * r + 1u]], n = raw < EDGE_UNSET ? raw : EDGE_UNSET - 1u;
    if (id >= nb_buffers)
      continue;
    const uint32_t have = row_table[id]; // (the ids of a buffer table are distinct: no other lane touches this word)
    if (have == EDGE_UNSET)
      row_table[id] = n;
    else if (have != n)
      changed++;
  }
  changed = wave_sum_u32(changed);
  if (lane == 0)
    wchg[wave] = changed;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    for (int w = 1; w < 16; w++)
      changed += wchg[w];
    const u64 total = start + carry, kept = total < max_edges ? total : max_edges, lost = (u64)dropped + (total - kept);
    stats[0] = (uint32_t)kept;
    stats[1] = lost < 0xFFFFFFFFull ? (uint32_t)lost : 0xFFFFFFFFu;
    stats[2] = calls + 1u;
    stats[3] = changed_before + changed;
  }
}

__global__ __launch_bounds__(TRK_THREADS) void k_edges_write(PairEdges in, const uint32_t *off, uint32_t max_edges, uint4 *edges)
{
  __shared__ uint32_t wcnt[TRK_THREADS / 64u];
  if (pair_block_idle(in))
    return;
  uint32_t ra, ia, rb, ib;
  const bool edge = pair_edge(in, ra, ia, rb, ib);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 bal = __ballot(edge);
  if (lane == 0)
    wcnt[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  u64 at = (u64)off[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + ballot_rank(bal, lane);
  for (int w = 0; w < wave; w++)
    at += wcnt[w];
  if (edge && at < max_edges)
    edges[at] = make_uint4(in.buf_tab[2u * ra], ia, in.buf_tab[2u * rb], ib);
}

__global__ __launch_bounds__(TRK_THREADS) void k_edges_hook(const uint4 *edges, const uint32_t *edge_count, uint32_t max_edges, const uint32_t *rank_tab, uint32_t nb_buffers,
                                                            const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows,
                                                            uint32_t *parent, uint32_t *ecnt)
{
  const uint32_t e = blockIdx.x * TRK_THREADS + threadIdx.x;
  uint32_t n = edge_count[0];
  n = n < max_edges ? n : max_edges;
  if (blockIdx.x * TRK_THREADS >= n)
    return; // (uniform over the workgroup)
  bool edge = e < n;
  uint32_t u = 0, v = 0;
  if (edge)
  {
    const uint4 rec = edges[e];
    edge = rec.x < nb_buffers && rec.z < nb_buffers;
    const uint32_t ra = edge ? rank_tab[rec.x] : TRK_NONE, rb = edge ? rank_tab[rec.z] : TRK_NONE; // (an absent buffer has no rank)
    edge = ra < nbufs && rb < nbufs;
    // (an edge that names a row that is not stored is no edge, so that no word outside the rows is touched)
    edge = edge && rec.y < buf_rows(buf_tab, rows_dev, ra, max_rows) && rec.w < buf_rows(buf_tab, rows_dev, rb, max_rows);
    if (edge)
      u = ra * node_stride + rec.y, v = rb * node_stride + rec.w;
  }
  count_block_edges(edge, blockIdx.x, ecnt);
  if (edge)
    union_nodes(parent, u, v);
}

static inline uint32_t edge_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + TRK_THREADS - 1u) / TRK_THREADS); }

extern "C" size_t vksift_hip_track_edges_scratch_u32(uint32_t nslots, uint32_t max_n) { return (size_t)nslots * edge_blocks(max_n); }

extern "C" int vksift_hip_append_track_edges(const uint8_t *records, uint64_t rec_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, const uint8_t *masks,
                                             uint64_t mask_slot_stride, const uint32_t *valid, uint32_t valid_stride, const uint32_t *slot_tab, uint32_t slot_tab_stride,
                                             uint32_t nslots, const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t max_rows, uint32_t *row_table,
                                             uint32_t nb_buffers, uint8_t *edges, uint32_t max_edges, uint32_t *stats, uint32_t *scratch, size_t scratch_u32,
                                             vksift_hip_stream s)
{
  const uint64_t nblocks = (uint64_t)nslots * edge_blocks(max_n);
  if (nslots == 0 || nbufs == 0 || max_n == 0 || max_rows == 0 || nb_buffers == 0 || max_edges == 0 || n_stride == 0 || slot_tab_stride < 2u ||
      (valid != nullptr && valid_stride == 0) || ((uintptr_t)records & 3u) || (rec_slot_stride & 3u) || ((uintptr_t)edges & 15u) || ((uintptr_t)scratch & 3u) ||
      (nslots > 1u && (rec_slot_stride < 16ull * max_n || (masks != nullptr && mask_slot_stride < max_n))) || nblocks > 0x7FFFFFFFull || scratch_u32 < nblocks)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)s;
  const uint32_t eblocks = edge_blocks(max_n);
  PairEdges in = {records, rec_slot_stride, n_dev, n_stride, max_n, masks, mask_slot_stride, valid, valid_stride, slot_tab, slot_tab_stride, buf_tab, nbufs, rows_dev, max_rows};
  // (a grid takes 65535 slots: a longer list goes in runs of that many, run r over the slots and the counts from r on)
  auto run = [&](uint32_t r) {
    PairEdges at = in;
    at.records += r * rec_slot_stride, at.n_dev += (size_t)r * n_stride, at.slot_tab += (size_t)r * slot_tab_stride;
    at.masks = masks ? masks + r * mask_slot_stride : nullptr, at.valid = valid ? valid + (size_t)r * valid_stride : nullptr;
    return at;
  };
  for (uint32_t r = 0; r < nslots; r += 65535u)
    k_edges_count<<<dim3(eblocks, nslots - r < 65535u ? nslots - r : 65535u), TRK_THREADS, 0, st>>>(run(r), scratch + (size_t)r * eblocks);
  k_edges_scan<<<1, 1024, 0, st>>>(scratch, (uint32_t)nblocks, buf_tab, nbufs, rows_dev, row_table, nb_buffers, max_edges, stats);
  for (uint32_t r = 0; r < nslots; r += 65535u)
    k_edges_write<<<dim3(eblocks, nslots - r < 65535u ? nslots - r : 65535u), TRK_THREADS, 0, st>>>(run(r), scratch + (size_t)r * eblocks, max_edges, (uint4 *)edges);
  return (int)hipGetLastError();
}

extern "C" int vksift_hip_build_tracks_from_edges(const uint8_t *edges, const uint32_t *edge_count, uint32_t max_edges, const uint32_t *rank_tab, uint32_t nb_buffers,
                                                  const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows,
                                                  uint32_t *node_words, uint8_t *tracks, uint64_t tracks_cap, uint32_t *stats, uint32_t *scratch, size_t scratch_u32,
                                                  vksift_hip_stream s)
{
  if (max_edges == 0 || nb_buffers == 0 || ((uintptr_t)edges & 15u) || tracks_args_check(nbufs, node_stride, max_rows, tracks, tracks_cap, scratch, scratch_u32) != 0)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)s;
  const TrackScratch t = track_scratch(scratch, nbufs, node_stride, max_rows);
  tracks_queue_init(buf_tab, rows_dev, node_stride, max_rows, t, st);
  k_edges_hook<<<edge_blocks(max_edges), TRK_THREADS, 0, st>>>((const uint4 *)edges, edge_count, max_edges, rank_tab, nb_buffers, buf_tab, nbufs, rows_dev, node_stride, max_rows,
                                                               t.parent, t.ecnt);
  tracks_queue_tail(buf_tab, nbufs, rows_dev, node_stride, max_rows, t, node_words, (uint32_t *)tracks, stats, st);
  return (int)hipGetLastError();
}
