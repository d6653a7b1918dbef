// tracks.h — what the two files that build feature tracks share (tracks.hip: from the pairs of a matching; track_edges.hip: from a stored edge list), each
// written once: the agent-scope accesses to the parent words, the find and the union of the lock-free union-find, the rule for a record being an edge, the
// per-node block mapping, the scratch layout of a build and the two host functions through which tracks.hip's launches around the hook are queued.
// DESIGN.md, "Tracks", holds the union-find and visibility argument: inside the hook and flatten launches every access to the parent words is an agent-scope
// atomic (relaxed load, CAS, relaxed store), since the XCDs' L2s are not coherent with each other; no lane ever waits for another workgroup.
#pragma once
#include "wave.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#define TRK_THREADS 256u
#define TRK_NONE 0xFFFFFFFFu
#define TRK_GROUP 64u /* buffers per presence launch: the bits of one presence word */
#define TRK_ECNT 64u  /* words the hook launch's edge count is spread over: thousands of atomic adds on ONE word cost more than the union-find */

typedef unsigned long long u64;

__device__ __forceinline__ uint32_t par_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// true: *p was `expect` and is `desired` now; otherwise `expect` holds what was found
__device__ __forceinline__ bool par_cas(uint32_t *p, uint32_t &expect, uint32_t desired)
{
  return __hip_atomic_compare_exchange_strong(p, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x. parent[v] <= v everywhere, so the walk strictly decreases until it meets a word that names itself. A stale "I am a root"
// is possible (the word was linked since); the caller's CAS on that word then fails and it walks on from what the CAS found.
template <bool SHORTEN> __device__ __forceinline__ uint32_t find_root(uint32_t *parent, uint32_t x)
{
  for (;;)
  {
    uint32_t p = par_load(parent + x);
    if (p == x)
      return x;
    if (SHORTEN)
    {
      // path halving, also through CAS: x is no root, its parent may only move to an ancestor, and never back to an older value
      const uint32_t gp = par_load(parent + p);
      if (gp != p)
        (void)par_cas(parent + x, p, gp);
    }
    x = p;
  }
}

// Link the larger root under the smaller: every component's root ends up its smallest member, whatever the schedule. A root stops being one
// exactly once, through a CAS on its own word; a failed CAS returns the parent it got, and the walk goes on from there.
__device__ __forceinline__ void union_nodes(uint32_t *parent, uint32_t u, uint32_t v)
{
  for (;;)
  {
    u = find_root<true>(parent, u);
    v = find_root<true>(parent, v);
    if (u == v)
      break;
    uint32_t hi = u > v ? u : v;
    const uint32_t lo = u > v ? v : u;
    uint32_t found = hi;
    if (par_cas(parent + hi, found, lo))
      break;
    u = found, v = lo;
  }
}

// the stored rows of the buffer of rank `rank` the launches touch
__device__ __forceinline__ uint32_t buf_rows(const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t rank, uint32_t max_rows)
{
  const uint32_t n = rows_dev[buf_tab[2u * rank + 1u]];
  return n < max_rows ? n : max_rows;
}

// what the per-node launches share: block b serves rows [256 (b % bpb), ...) of the buffer of rank first_rank + b / bpb. Returns the node index, or
// TRK_NONE for a lane without a stored row
__device__ __forceinline__ uint32_t block_node(const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t first_rank, uint32_t bpb, uint32_t node_stride, uint32_t max_rows,
                                               uint32_t &rank, uint32_t &row)
{
  rank = first_rank + blockIdx.x / bpb;
  row = (blockIdx.x % bpb) * TRK_THREADS + threadIdx.x;
  return row < buf_rows(buf_tab, rows_dev, rank, max_rows) ? rank * node_stride + row : TRK_NONE;
}

// The records of the pairs of a matching as the launches with a grid of (blocks of 256 records, slots) read them: the arguments vksift_hip_build_tracks
// documents (include/vksift_hip.h).
struct PairEdges
{
  const uint8_t *records;
  uint64_t rec_slot_stride;
  const uint32_t *n_dev;
  uint32_t n_stride, max_n;
  const uint8_t *masks;
  uint64_t mask_slot_stride;
  const uint32_t *valid;
  uint32_t valid_stride;
  const uint32_t *slot_tab;
  uint32_t slot_tab_stride;
  const uint32_t *buf_tab;
  uint32_t nbufs;
  const uint32_t *rows_dev;
  uint32_t max_rows;
};

// the slot's records below 256 blockIdx.x are none, or its pair is not valid: nothing of this workgroup is an edge (uniform over the workgroup)
__device__ __forceinline__ bool pair_block_idle(const PairEdges &in)
{
  const uint32_t p = blockIdx.y;
  uint32_t n = in.n_dev[(size_t)p * in.n_stride];
  n = n < in.max_n ? n : in.max_n;
  return blockIdx.x * TRK_THREADS >= n || (in.valid != nullptr && in.valid[(size_t)p * in.valid_stride] == 0);
}

// is record 256 blockIdx.x + threadIdx.x of slot blockIdx.y an edge (of a workgroup that is not idle), and between which ranks and rows
__device__ __forceinline__ bool pair_edge(const PairEdges &in, uint32_t &ra, uint32_t &ia, uint32_t &rb, uint32_t &ib)
{
  const uint32_t p = blockIdx.y, e = blockIdx.x * TRK_THREADS + threadIdx.x;
  uint32_t n = in.n_dev[(size_t)p * in.n_stride];
  n = n < in.max_n ? n : in.max_n;
  ra = in.slot_tab[(size_t)p * in.slot_tab_stride], rb = in.slot_tab[(size_t)p * in.slot_tab_stride + 1u];
  bool edge = e < n && ra < in.nbufs && rb < in.nbufs;
  if (edge && in.masks != nullptr)
    edge = in.masks[p * in.mask_slot_stride + e] == 1u;
  ia = ib = 0;
  if (edge)
  {
    const uint32_t *rec = (const uint32_t *)(in.records + p * in.rec_slot_stride + (uint64_t)e * 16u);
    ia = rec[0], ib = rec[1];
    // (a record of the library's own producers always names stored rows; anything else is no edge, so that no word outside the rows is touched)
    edge = ia < buf_rows(in.buf_tab, in.rows_dev, ra, in.max_rows) && ib < buf_rows(in.buf_tab, in.rows_dev, rb, in.max_rows);
  }
  return edge;
}

// the workgroup's edges into the counters the scan launch adds up
__device__ __forceinline__ void count_block_edges(bool edge, uint32_t block, uint32_t *ecnt)
{
  const uint32_t in_block = (uint32_t)__syncthreads_count(edge);
  if (threadIdx.x == 0 && in_block)
    atomicAdd(ecnt + (block & (TRK_ECNT - 1u)), in_block);
}

static inline uint64_t trk_blocks_per_buffer(uint32_t rows) { return ((uint64_t)rows + TRK_THREADS - 1u) / TRK_THREADS; }

// where a build keeps what in its scratch (vksift_hip_tracks_scratch_u32 words), and the grid of its per-node launches
struct TrackScratch
{
  u64 *bits;
  uint32_t *parent, *len, *nbuf, *bsum, *ecnt;
  uint32_t bpb, nblocks;
};
static inline TrackScratch track_scratch(uint32_t *scratch, uint32_t nbufs, uint32_t node_stride, uint32_t max_rows)
{
  const uint64_t nodes = (uint64_t)nbufs * node_stride;
  TrackScratch t;
  t.bpb = (uint32_t)trk_blocks_per_buffer(max_rows);
  t.nblocks = nbufs * t.bpb;
  t.bits = (u64 *)scratch;
  t.parent = scratch + 2u * nodes, t.len = t.parent + nodes, t.nbuf = t.len + nodes, t.bsum = t.nbuf + nodes, t.ecnt = t.bsum + 3u * (size_t)t.nblocks;
  return t;
}

// tracks.hip. The arguments every entry that builds tracks refuses (hipErrorInvalidValue) or takes (0) before anything is launched
int tracks_args_check(uint32_t nbufs, uint32_t node_stride, uint32_t max_rows, const uint8_t *tracks, uint64_t tracks_cap, const uint32_t *scratch, size_t scratch_u32);
// k_tracks_init: every stored row its own parent, its words and the edge counters zero
void tracks_queue_init(const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, const TrackScratch &t, hipStream_t st);
// k_tracks_flatten ... k_tracks_label: from the parent words the hook launches left to the node words, the track records and the statistics
void tracks_queue_tail(const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, const TrackScratch &t, uint32_t *node_words,
                       uint32_t *tracks, uint32_t *stats, hipStream_t st);
