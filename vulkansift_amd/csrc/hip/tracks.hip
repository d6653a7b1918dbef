// tracks.hip — multi-view feature tracks: the connected components of the graph whose nodes are the rows of the SIFT buffers of a pair list
// and whose edges are the pairs' match records (vksift_hip_build_tracks; no counterpart in the reference, whose callers download every
// pair's matches and run a union-find on the host). DESIGN.md, "Tracks", holds the argument; the header (include/vksift_hip.h) the contract.
//
// Node index = rank * node_stride + row, rank = position of the buffer in buf_tab (increasing gpu_buffer_id), so index order is the order
// (gpu_buffer_id, row). A launch sequence on one stream; every phase that reads another phase's plain stores is a launch of its own:
//   k_tracks_init     every stored row of a participating buffer its own parent, its words zero
//   k_tracks_hook     one lane per record: find both roots, CAS the larger root's own word to the smaller (lock-free union-find)
//   k_tracks_flatten  every node finds its root, stores it as its parent and adds 1 to the root's length
//   k_tracks_presence (per group of 64 buffers) the member's buffer bit into the root's 64-bit presence word
//   k_tracks_fold     (per group) roots add the popcount of their presence word to nb_buffers and clear it; the last one also counts the
//                     tracks (roots of length >= 2), the conflicting ones and the members of every block
//   k_tracks_scan     exclusive scan of the block counts, and the four statistics (one workgroup)
//   k_tracks_number   block scan + block offset = track number: the roots' words and the track records
//   k_tracks_label    every other node copies its root's word
// Inside k_tracks_hook and k_tracks_flatten every access to the parent words is an agent-scope atomic (relaxed load, CAS, relaxed store):
// the XCDs' L2s are not coherent with each other. No lane ever waits for another workgroup: a failed CAS means another lane has linked
// that root, which is progress; finds walk strictly decreasing indices.
#include "vksift_hip.h"
#include "tracks.h"

#include <hip/hip_runtime.h>

__global__ __launch_bounds__(TRK_THREADS) void k_tracks_init(const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t bpb, uint32_t node_stride, uint32_t max_rows,
                                                             uint32_t *parent, uint32_t *len, uint32_t *nbuf, u64 *bits, uint32_t *ecnt)
{
  uint32_t rank, row;
  const uint32_t node = block_node(buf_tab, rows_dev, 0, bpb, node_stride, max_rows, rank, row);
  if (blockIdx.x == 0 && threadIdx.x < TRK_ECNT)
    ecnt[threadIdx.x] = 0;
  if (node == TRK_NONE)
    return;
  parent[node] = node;
  len[node] = 0;
  nbuf[node] = 0;
  bits[node] = 0;
}

__global__ __launch_bounds__(TRK_THREADS) void k_tracks_hook(const uint8_t *records, uint64_t rec_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n,
                                                             const uint8_t *masks, uint64_t mask_slot_stride, const uint32_t *valid, uint32_t valid_stride,
                                                             const uint32_t *slot_tab, uint32_t slot_tab_stride, const uint32_t *buf_tab, uint32_t nbufs,
                                                             const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, uint32_t *parent, uint32_t *ecnt)
{
  const PairEdges in = {records, rec_slot_stride, n_dev, n_stride, max_n, masks, mask_slot_stride, valid, valid_stride, slot_tab, slot_tab_stride, buf_tab, nbufs, rows_dev, max_rows};
  if (pair_block_idle(in))
    return;
  uint32_t ra, ia, rb, ib;
  const bool edge = pair_edge(in, ra, ia, rb, ib);
  count_block_edges(edge, blockIdx.y * gridDim.x + blockIdx.x, ecnt);
  if (edge)
    union_nodes(parent, ra * node_stride + ia, rb * node_stride + ib);
}

__global__ __launch_bounds__(TRK_THREADS) void k_tracks_flatten(const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t bpb, uint32_t node_stride, uint32_t max_rows,
                                                                uint32_t *parent, uint32_t *len)
{
  uint32_t rank, row;
  const uint32_t node = block_node(buf_tab, rows_dev, 0, bpb, node_stride, max_rows, rank, row);
  if (node == TRK_NONE)
    return;
  // other lanes of this launch store roots over the words this walk reads: a root is an ancestor like any other, the walk still ends at the root
  const uint32_t root = find_root<false>(parent, node);
  __hip_atomic_store(parent + node, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(len + root, 1u);
}

__global__ __launch_bounds__(TRK_THREADS) void k_tracks_presence(const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t first_rank, uint32_t bpb, uint32_t node_stride,
                                                                 uint32_t max_rows, const uint32_t *parent, const uint32_t *len, u64 *bits)
{
  uint32_t rank, row;
  const uint32_t node = block_node(buf_tab, rows_dev, first_rank, bpb, node_stride, max_rows, rank, row);
  if (node == TRK_NONE)
    return;
  const uint32_t root = parent[node];
  if (len[root] >= 2u)
    atomicOr(bits + root, 1ull << (rank & (TRK_GROUP - 1u)));
}

// is this lane's node the root of a track
__device__ __forceinline__ bool is_track_root(uint32_t node, const uint32_t *parent, const uint32_t *len) { return node != TRK_NONE && parent[node] == node && len[node] >= 2u; }

__global__ __launch_bounds__(TRK_THREADS) void k_tracks_fold(const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t bpb, uint32_t node_stride, uint32_t max_rows,
                                                             const uint32_t *parent, const uint32_t *len, uint32_t *nbuf, u64 *bits, uint32_t *bsum)
{
  __shared__ uint32_t wfeat[TRK_THREADS / 64u];
  uint32_t rank, row;
  const uint32_t node = block_node(buf_tab, rows_dev, 0, bpb, node_stride, max_rows, rank, row);
  const bool track = is_track_root(node, parent, len);
  uint32_t nb = 0;
  if (track)
  {
    const u64 b = bits[node];
    nb = nbuf[node] + (uint32_t)__popcll(b);
    if (b)
      nbuf[node] = nb, bits[node] = 0;
  }
  if (bsum != nullptr)
  {
    // the last fold: the block's tracks, conflicting tracks and members, three words per block for the scan launch to add up
    const uint32_t l = track ? len[node] : 0u;
    const uint32_t cnt = (uint32_t)__syncthreads_count(track), conf = (uint32_t)__syncthreads_count(track && l > nb);
    const uint32_t feat = wave_sum_u32(l);
    if ((threadIdx.x & 63u) == 0)
      wfeat[threadIdx.x >> 6] = feat;
    __syncthreads();
    if (threadIdx.x == 0)
    {
      bsum[blockIdx.x] = cnt;
      bsum[gridDim.x + blockIdx.x] = conf;
      bsum[2u * gridDim.x + blockIdx.x] = wfeat[0] + wfeat[1] + wfeat[2] + wfeat[3];
    }
  }
}

// bsum[0 .. nblocks) becomes its exclusive prefix sum; stats: the total, the sums of the two arrays behind it, and the sum of the edge counters. One
// workgroup of 1024.
__global__ __launch_bounds__(1024) void k_tracks_scan(uint32_t *bsum, uint32_t nblocks, const uint32_t *ecnt, uint32_t *stats)
{
  __shared__ uint32_t wsum[17], wtot[3][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0, conf = 0, feat = 0;
  for (uint32_t base = 0; base < nblocks; base += 1024u)
  {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nblocks ? bsum[i] : 0u;
    conf += i < nblocks ? bsum[nblocks + i] : 0u;
    feat += i < nblocks ? bsum[2u * nblocks + i] : 0u;
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
      bsum[i] = carry + wsum[wave] + incl - v;
    carry += wsum[16];
    __syncthreads();
  }
  conf = wave_sum_u32(conf), feat = wave_sum_u32(feat);
  const uint32_t edges = wave_sum_u32(threadIdx.x < TRK_ECNT ? ecnt[threadIdx.x] : 0u);
  if (lane == 0)
    wtot[0][wave] = conf, wtot[1][wave] = feat, wtot[2][wave] = edges;
  __syncthreads();
  if (threadIdx.x < 3u)
  {
    uint32_t t = 0;
    for (int w = 0; w < 16; w++)
      t += wtot[threadIdx.x][w];
    stats[1u + threadIdx.x] = t;
  }
  if (threadIdx.x == 0)
    stats[0] = carry;
}

__global__ __launch_bounds__(TRK_THREADS) void k_tracks_number(const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t bpb, uint32_t node_stride, uint32_t max_rows,
                                                               const uint32_t *parent, const uint32_t *len, const uint32_t *nbuf, const uint32_t *bsum,
                                                               uint32_t *node_words, uint32_t *tracks)
{
  __shared__ uint32_t wcnt[TRK_THREADS / 64u];
  uint32_t rank, row;
  const uint32_t node = block_node(buf_tab, rows_dev, 0, bpb, node_stride, max_rows, rank, row);
  const bool track = is_track_root(node, parent, len);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 bal = __ballot(track);
  if (lane == 0)
    wcnt[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t t = bsum[blockIdx.x] + ballot_rank(bal, lane);
  for (int w = 0; w < wave; w++)
    t += wcnt[w];
  if (track)
  {
    uint32_t *rec = tracks + (size_t)t * 4u;
    rec[0] = buf_tab[2u * rank], rec[1] = row, rec[2] = len[node], rec[3] = nbuf[node];
    node_words[node] = t;
  }
  else if (node != TRK_NONE && parent[node] == node)
    node_words[node] = TRK_NONE;
}

__global__ __launch_bounds__(TRK_THREADS) void k_tracks_label(const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t bpb, uint32_t node_stride, uint32_t max_rows,
                                                              const uint32_t *parent, uint32_t *node_words)
{
  uint32_t rank, row;
  const uint32_t node = block_node(buf_tab, rows_dev, 0, bpb, node_stride, max_rows, rank, row);
  if (node == TRK_NONE)
    return;
  const uint32_t root = parent[node];
  if (root != node)
    node_words[node] = node_words[root]; // (the roots' words are the previous launch's: no lane of this one writes them)
}

extern "C" size_t vksift_hip_tracks_scratch_u32(uint32_t nbufs, uint32_t node_stride)
{
  const uint64_t nodes = (uint64_t)nbufs * node_stride;
  return (size_t)(5u * nodes + 3u * (uint64_t)nbufs * trk_blocks_per_buffer(node_stride) + TRK_ECNT + 2u);
}

int tracks_args_check(uint32_t nbufs, uint32_t node_stride, uint32_t max_rows, const uint8_t *tracks, uint64_t tracks_cap, const uint32_t *scratch, size_t scratch_u32)
{
  const uint64_t nodes = (uint64_t)nbufs * node_stride;
  if (nbufs == 0 || max_rows == 0 || max_rows > node_stride || nodes >= 0xFFFFFFFFull || ((uintptr_t)tracks & 3u) || ((uintptr_t)scratch & 7u) ||
      tracks_cap < (uint64_t)nbufs * max_rows / 2u || scratch_u32 < vksift_hip_tracks_scratch_u32(nbufs, node_stride) ||
      (uint64_t)nbufs * trk_blocks_per_buffer(max_rows) > 0x7FFFFFFFull)
    return (int)hipErrorInvalidValue;
  return 0;
}

void tracks_queue_init(const uint32_t *buf_tab, const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, const TrackScratch &t, hipStream_t st)
{
  k_tracks_init<<<t.nblocks, TRK_THREADS, 0, st>>>(buf_tab, rows_dev, t.bpb, node_stride, max_rows, t.parent, t.len, t.nbuf, t.bits, t.ecnt);
}

void tracks_queue_tail(const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, const TrackScratch &t, uint32_t *node_words,
                       uint32_t *tracks, uint32_t *stats, hipStream_t st)
{
  const uint32_t bpb = t.bpb, nblocks = t.nblocks;
  k_tracks_flatten<<<nblocks, TRK_THREADS, 0, st>>>(buf_tab, rows_dev, bpb, node_stride, max_rows, t.parent, t.len);
  for (uint32_t g = 0; g < nbufs; g += TRK_GROUP)
  {
    const uint32_t nb = nbufs - g < TRK_GROUP ? nbufs - g : TRK_GROUP;
    k_tracks_presence<<<nb * bpb, TRK_THREADS, 0, st>>>(buf_tab, rows_dev, g, bpb, node_stride, max_rows, t.parent, t.len, t.bits);
    k_tracks_fold<<<nblocks, TRK_THREADS, 0, st>>>(buf_tab, rows_dev, bpb, node_stride, max_rows, t.parent, t.len, t.nbuf, t.bits, g + TRK_GROUP >= nbufs ? t.bsum : nullptr);
  }
  k_tracks_scan<<<1, 1024, 0, st>>>(t.bsum, nblocks, t.ecnt, stats);
  k_tracks_number<<<nblocks, TRK_THREADS, 0, st>>>(buf_tab, rows_dev, bpb, node_stride, max_rows, t.parent, t.len, t.nbuf, t.bsum, node_words, tracks);
  k_tracks_label<<<nblocks, TRK_THREADS, 0, st>>>(buf_tab, rows_dev, bpb, node_stride, max_rows, t.parent, node_words);
}

extern "C" int vksift_hip_build_tracks(const uint8_t *records, uint64_t rec_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, const uint8_t *masks,
                                       uint64_t mask_slot_stride, const uint32_t *valid, uint32_t valid_stride, const uint32_t *slot_tab, uint32_t slot_tab_stride,
                                       uint32_t nslots, const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows,
                                       uint32_t *node_words, uint8_t *tracks, uint64_t tracks_cap, uint32_t *stats, uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s)
{
  if (nslots == 0 || max_n == 0 || n_stride == 0 || slot_tab_stride < 2u || (valid != nullptr && valid_stride == 0) || ((uintptr_t)records & 3u) || (rec_slot_stride & 3u) ||
      (nslots > 1u && (rec_slot_stride < 16ull * max_n || (masks != nullptr && mask_slot_stride < max_n))) ||
      tracks_args_check(nbufs, node_stride, max_rows, tracks, tracks_cap, scratch, scratch_u32) != 0)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)s;
  const TrackScratch t = track_scratch(scratch, nbufs, node_stride, max_rows);
  tracks_queue_init(buf_tab, rows_dev, node_stride, max_rows, t, st);
  const uint32_t eblocks = (max_n + TRK_THREADS - 1u) / TRK_THREADS;
  for (uint32_t r = 0; r < nslots; r += 65535u)
  {
    const uint32_t n = nslots - r < 65535u ? nslots - r : 65535u;
    k_tracks_hook<<<dim3(eblocks, n), TRK_THREADS, 0, st>>>(records + r * rec_slot_stride, rec_slot_stride, n_dev + (size_t)r * n_stride, n_stride, max_n,
                                                            masks ? masks + r * mask_slot_stride : nullptr, mask_slot_stride, valid ? valid + (size_t)r * valid_stride : nullptr,
                                                            valid_stride, slot_tab + (size_t)r * slot_tab_stride, slot_tab_stride, buf_tab, nbufs, rows_dev, node_stride,
                                                            max_rows, t.parent, t.ecnt);
  }
  tracks_queue_tail(buf_tab, nbufs, rows_dev, node_stride, max_rows, t, node_words, (uint32_t *)tracks, stats, st);
  return (int)hipGetLastError();
}
