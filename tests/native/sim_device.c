/*
 * sim_device.c — a simulated device behind the whole host library (tests/test_detect_plan.py; no GPU). It defines every vksift_hip_*
 * symbol that csrc/host/ needs, computes nothing and RECORDS: one log line per launcher, copy, memset, event record and stream wait,
 * with the stream it went to and a digest of every argument. tests/native/plan_harness.c drives the public API over it; the scenarios
 * and every assertion are in Python.
 *
 * Memory. Device addresses are fake (a range no process can map), handed out monotonically and never dereferenced: a full-size instance
 * costs nothing. Pinned memory is real (the host writes images into it and reads counters out of it) and stays mapped — poisoned for the
 * address sanitizer once freed — until sim_finish(), so that an address names one block for the whole run. A ledger holds live and dead
 * blocks.
 * Digests. Pointer words are recognised BY SCANNING: every aligned 8-byte word of an argument (or of an array reached through one:
 * vksift_hip_OctaveJob[], plane lists, taps, vksift_hip_DenseRows) whose value lies inside a ledger block is replaced by (block index,
 * offset) before it is hashed — no per-field knowledge, and two runs whose addresses differ compare equal. Structures the host fills
 * field by field (vksift_hip_Plane, vksift_hip_PlaceOctave: their padding is not initialised) are digested field by field. A host pointer
 * outside the ledger (caller memory, a stack table) is digested by content where the shim's contract gives its length, else as a tag.
 * Arguments that are host-side bounds on counts the device holds go into a second digest (T()): max_na, max_nb and nb_exact of
 * vksift_hip_match_2nn_async, and max_rows of EVERY launcher that takes one (vksift_hip_gather_sections, vksift_hip_pack_features,
 * vksift_hip_root_descriptors) — by the contract of include/vksift_hip.h each of them sizes a grid and nothing else. How tight they are
 * follows from which detections the host has seen complete, which a replayed and a directly queued detection may legitimately differ in
 * on a busy device; idle, the tests compare this digest as strictly as the other. Every other argument is an input (V(), P(), A()).
 * Results. A device-to-host copy zero-fills its destination; vksift_hip_post_words and the posting of the dense descriptor launch write
 * `sim_counts` into every counter word, so that the stages behind a detection plan real launches.
 * Time. Idle mode: events complete at once. Busy mode: an event stays busy until its stream (or it) is synchronised or sim_drain().
 * Capture. vksift_hip_capture_begin opens a capture on a stream; a stream that waits on an event recorded inside it joins; operations
 * on capturing streams are stored instead of issued ("cop" lines); capture_end yields an exec; graph_launch issues the stored records
 * again ("gop" lines) and runs their effects.
 * Hard checks ("VIOLATION" lines, exit status through sim_violations):
 *   C1 every block an operation names is live when it is issued — for a graph at every launch;
 *   C2 no sync / busy / elapsed query touches a capturing stream or an event of the open capture; at capture_end every joined stream
 *      has rejoined; no stream outside a capture waits on an event whose last record was inside a finished capture; no capture is
 *      open when an API call returns (sim_api_return);
 *   C3 no exec launched or destroyed after its destruction, none destroyed on a busy GPU before the host has seen its last launch complete
 *      (a wait for a later event or a sync of its stream); a clean ledger after vksift_destroyInstance (sim_report_ledger).
 * Fault injection: sim_fail_in = k makes the k-th counted call from now (every line that starts with "#") return an error; sim_fail_then = j, set
 * with it, makes the j-th counted call behind that failure fail as well (an error exit whose own device call fails).
 *
 * The stages behind a matching (tests/test_pair_plan.py). Nothing below changes a log line or a digest unless its switch is set:
 *   Pointer arguments by role (sim_roles). For the copies and for the launchers of the matcher, the in-place passes and the pair stages, the
 *      operation's line is followed by "args NAME arg=bN+OFFSET:r|w:EXTENT ...": per pointer argument the ledger block, the offset, the role
 *      (`w` iff the prototype of include/vksift_hip.h has no `const`) and the bytes it may touch (0: the header states none). "-" : not a
 *      ledger address (NULL, caller memory).
 *   C4 extents (sim_roles). The extent is derived from the launch's own scalar arguments as include/vksift_hip.h words it (stride x slots,
 *      words x slots x 4, max_n x element, scratch_u32 x 4, nbufs x node_stride x 4, tracks_cap x 16 ...); offset + extent beyond the block is
 *      a VIOLATION, and so is, with more than one slot, a stride below what a slot may hold (max_n x element).
 *   C5 pinned inputs stay put (sim_roles, busy mode). An operation with a read argument inside a pinned block stores a hash of the bytes it
 *      will read; the hash is checked when the host first sees the operation complete (a synchronisation of its stream or of a later event
 *      on it, of a stream that waited for it, or sim_drain). A difference is a VIOLATION: the host rewrote a table in flight.
 *   Late posts (sim_late_posts, busy mode). vksift_hip_post_words and the device-to-host copies fill their destination with SIM_POISON when
 *      issued and with the real value only at the synchronisation that covers them: an accessor that returns the poison read before it
 *      waited. A pitched two-dimensional copy is filled row by row, the gaps between its rows left alone.
 *   Counted allocations (sim_count_allocs). vksift_hip_malloc, vksift_hip_host_malloc and vksift_hip_event_create are counted calls: fault
 *      injection can refuse them.
 *   Balanced ranges. vksift_hip_range_push / _pop are balanced whenever an API call returns (sim_api_return; C2).
 */
#include "vksift_hip.h"

#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)(p), (void)(n))
#define UNPOISON(p, n) ((void)(p), (void)(n))
#endif

#define SIM_ERR 719 /* what an injected failure returns */
#define MAX_BLOCKS 16384
#define MAX_STREAMS 64
#define MAX_EVENTS 1024
#define MAX_EXECS 8192
#define MAX_REC_BLOCKS 96

/* ------------------------------------------------------------------------------------------------ switches (set by the harness) */
int sim_busy_mode;           /* 1: events stay busy until synchronised or drained */
int sim_covered = 1;         /* answer of the optional launchers: 1 launched, 0 "not covered" (-1) */
uint32_t sim_counts;         /* value the counter postings write */
uint64_t sim_fail_in;        /* 1: the next counted call fails */
uint64_t sim_fail_then;      /* j: ... and the j-th counted call behind that failure too (0: none) */
uint64_t sim_violations;
int sim_roles;               /* 1: "args" lines, C4, and (busy mode) C5 */
int sim_late_posts;          /* 1 (busy mode): postings and device-to-host copies arrive at the synchronisation that covers them */
int sim_count_allocs;        /* 1: allocations and event creations are counted calls */
#define SIM_POISON 0xD0D0D0D0u
static uint64_t call_no;
static int range_depth;
static bool counted(const char *name);

/* ------------------------------------------------------------------------------------------------ ledger */
typedef struct
{
  uintptr_t base;
  size_t bytes;
  char kind; /* D device, H pinned */
  bool live;
} Block;
static Block blocks[MAX_BLOCKS];
static uint32_t n_blocks;
static uintptr_t next_fake = (uintptr_t)1 << 60;
static uint64_t device_live;

typedef struct
{
  bool live;
  int cap;              /* capture it belongs to (0: none) */
  uint64_t seq;         /* operations and records issued to it */
  uint64_t joined_upto; /* capture: the origin side has waited for everything up to here */
  uint64_t done_upto;   /* busy mode: the host has seen everything up to here complete */
  bool busy;
} Stream;
typedef struct
{
  bool live, busy, recorded;
  int cap; /* capture its last record was in (0: none) */
  int stream;
  uint64_t seq;
} Event;
static Stream streams[MAX_STREAMS];
static Event events[MAX_EVENTS];
static uint32_t n_streams, n_events;

typedef struct
{
  char name[28];
  int stream;
  uint64_t digest;
  uint64_t bounds; /* digest of the arguments that are host-side BOUNDS on device-side counts (T()): they follow what the host happens to know */
  uint32_t nblk;
  uint32_t blk[MAX_REC_BLOCKS];
  uint32_t *fill; /* effect when it is issued or replayed: the fill_bytes bytes at fill become sim_counts per word (fill_counts) or 0 */
  size_t fill_bytes;
  size_t fill_pitch; /* 0: one run of fill_bytes; else fill_rows rows of fill_bytes, fill_pitch apart (a pitched copy: the gaps stay as they are) */
  size_t fill_rows;
  bool fill_counts;
} Record;
typedef struct
{
  bool live, destroyed;
  Record *recs;
  uint32_t n;
  int last_stream; /* its last launch on a busy GPU: stream and position (-1: none) */
  uint64_t last_seq;
} Exec;
static Exec execs[MAX_EXECS];
static uint32_t n_execs;
static int open_cap, open_origin = -1, n_caps; /* the open capture's id (0: none) and origin stream */
static bool cap_invalid;                      /* a call failed inside the open capture: like the real runtime's, it is invalidated and its end fails */
static Record *cap_recs;
static uint32_t cap_n, cap_room;

static void violation(const char *rule, const char *what, long a, long b)
{
  sim_violations++;
  printf("VIOLATION %s %s %ld %ld\n", rule, what, a, b);
}

static int block_of(uintptr_t v)
{
  if (v < 4096)
    return -1;
  for (uint32_t i = n_blocks; i-- > 0;) /* (pinned memory stays mapped: ranges never overlap) */
    if (v >= blocks[i].base && v <= blocks[i].base + blocks[i].bytes)
      return (int)i;
  return -1;
}

static void *acquire(char kind, size_t bytes)
{
  if (n_blocks == MAX_BLOCKS)
    return NULL;
  if (sim_count_allocs && counted("alloc"))
    return NULL;
  Block *b = &blocks[n_blocks];
  if (kind == 'D')
  {
    b->base = next_fake;
    next_fake += (((uintptr_t)bytes + 0xfff) & ~(uintptr_t)0xfff) + 0x1000;
    device_live += bytes;
  }
  else
  {
    void *p = calloc(1, bytes ? bytes : 1);
    if (!p)
      return NULL;
    b->base = (uintptr_t)p;
  }
  b->bytes = bytes, b->kind = kind, b->live = true;
  if (sim_count_allocs)
    printf("#%llu ", (unsigned long long)call_no);
  printf("alloc %c b%u %zu\n", kind, n_blocks, bytes);
  n_blocks++;
  return (void *)b->base;
}

static void release(char kind, void *p)
{
  if (!p)
    return;
  const int i = block_of((uintptr_t)p);
  if (i < 0 || !blocks[i].live || blocks[i].kind != kind || blocks[i].base != (uintptr_t)p)
    return violation("C3", "bad free", i, kind);
  blocks[i].live = false;
  printf("free %c b%d %zu\n", kind, i, blocks[i].bytes);
  if (kind == 'D')
    device_live -= blocks[i].bytes;
  else
    POISON(p, blocks[i].bytes ? blocks[i].bytes : 1);
}

void *vksift_hip_malloc(size_t bytes) { return acquire('D', bytes); }
void vksift_hip_free(void *p) { release('D', p); }
void *vksift_hip_host_malloc(size_t bytes) { return acquire('H', bytes); }
void vksift_hip_host_free(void *p) { release('H', p); }
int vksift_hip_host_register(void *p, size_t bytes) { return (void)p, (void)bytes, 0; }
int vksift_hip_host_unregister(void *p) { return (void)p, 0; }
int vksift_hip_is_pinned(const void *p)
{
  const int i = block_of((uintptr_t)p);
  return i >= 0 && blocks[i].kind == 'H' && blocks[i].live;
}
size_t vksift_hip_device_free_mem(void) { return (size_t)(((uint64_t)288 << 30) - device_live); }
int vksift_hip_init(void) { return 0; }
uint32_t vksift_hip_abi_version(void) { return VKSIFT_HIP_ABI_VERSION; }
int vksift_hip_device_count(void) { return 1; }
int vksift_hip_device_name(int idx, char *out256) { return (void)idx, snprintf(out256, 256, "simulated device"), 0; }
int vksift_hip_set_device(int idx) { return idx == 0 ? 0 : 1; }
const char *vksift_hip_error_string(int err) { return err == SIM_ERR ? "injected failure" : "simulated error"; }
void vksift_hip_range_push(const char *name) { (void)name, range_depth++; }
void vksift_hip_range_pop(void)
{
  if (--range_depth < 0)
  {
    sim_violations++, range_depth = 0;
    printf("VIOLATION C2 a range is popped that was not pushed\n");
  }
}
int vksift_hip_tune_get(int knob) { return (void)knob, 0; }
int vksift_hip_blur_form(vksift_hip_Plane src, vksift_hip_Plane dst, uint32_t ntaps, uint32_t batch) { return (void)src, (void)dst, (void)ntaps, (void)batch, sim_covered ? 1 : 0; }
size_t vksift_hip_match_scratch_u32(uint32_t na, uint32_t nb) { return VKSIFT_HIP_MATCH_SCRATCH_U32(na, nb); }
size_t vksift_hip_ransac_scratch_u32(uint32_t nslots, uint32_t nb_hypotheses) { return 64u + (size_t)nslots * nb_hypotheses; }
size_t vksift_hip_guided_scratch_u32(uint32_t nslots, uint32_t max_n) { return (size_t)nslots * max_n * 8u; }
size_t vksift_hip_tracks_scratch_u32(uint32_t nbufs, uint32_t node_stride)
{
  return (size_t)(5u * (uint64_t)nbufs * node_stride + 3u * (uint64_t)nbufs * (((uint64_t)node_stride + 255u) / 256u) + 64u + 2u);
}

/* ------------------------------------------------------------------------------------------------ streams and events */
static int stream_id(vksift_hip_stream s, const char *who)
{
  const long i = (Stream *)s - streams;
  if (!s || (uintptr_t)s < (uintptr_t)streams || i >= (long)n_streams || !streams[i].live)
  {
    violation("C3", who, -1, 0);
    return -1;
  }
  return (int)i;
}
static int event_id(vksift_hip_event e, const char *who)
{
  const long i = (Event *)e - events;
  if (!e || (uintptr_t)e < (uintptr_t)events || i >= (long)n_events || !events[i].live)
  {
    violation("C3", who, -1, 0);
    return -1;
  }
  return (int)i;
}
/* a counted call: its number is printed in front of its line; true: it is the one that fails */
static bool counted(const char *name)
{
  call_no++;
  if (sim_fail_in && --sim_fail_in == 0)
  {
    printf("#%llu FAIL %s\n", (unsigned long long)call_no, name);
    sim_fail_in = sim_fail_then, sim_fail_then = 0;
    cap_invalid = open_cap != 0;
    return true;
  }
  return false;
}

vksift_hip_stream vksift_hip_stream_create(void)
{
  if (n_streams == MAX_STREAMS)
    return NULL;
  memset(&streams[n_streams], 0, sizeof(Stream));
  streams[n_streams].live = true;
  return &streams[n_streams++];
}
void vksift_hip_stream_destroy(vksift_hip_stream s)
{
  const int i = s ? stream_id(s, "stream destroyed twice") : -1;
  if (i >= 0)
    streams[i].live = false;
}
vksift_hip_event vksift_hip_event_create(void)
{
  if (n_events == MAX_EVENTS)
    return NULL;
  if (sim_count_allocs)
  {
    if (counted("event_create"))
      return NULL;
    printf("#%llu evcreate e%u\n", (unsigned long long)call_no, n_events);
  }
  memset(&events[n_events], 0, sizeof(Event));
  events[n_events].live = true;
  return &events[n_events++];
}
void vksift_hip_event_destroy(vksift_hip_event e)
{
  const int i = e ? event_id(e, "event destroyed twice") : -1;
  if (i >= 0)
    events[i].live = false;
}

/* What waits for the host to SEE an operation complete (sim_roles, sim_late_posts; busy mode): the hash of a pinned input (C5) and the real
 * value of a late post, per stream position; and the stream waits, through which seeing one stream pass a position shows another's. */
typedef struct
{
  int stream;
  uint64_t seq;
  char kind; /* c: check the hash; f: fill; 0: done */
  void *p;
  size_t n;
  uint64_t hash;
  bool counts;
  char name[28];
  size_t pitch, rows; /* a fill of `rows` rows of n bytes (pitch 0: one run) */
} Pending;
typedef struct
{
  int stream, on;
  uint64_t at, upto;
} Dep;
static Pending *pend;
static Dep *deps;
static uint32_t n_pend, room_pend, n_deps, room_deps;

static uint64_t hash_bytes(const void *p, size_t n)
{
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++)
    h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
  return h;
}
static int block_of(uintptr_t v);
static void fill_run(uint32_t *dst, size_t bytes, bool counts, uint32_t poison);
static void fill_words(uint32_t *dst, size_t bytes, size_t pitch, size_t rows, bool counts, uint32_t poison)
{
  const int bi = block_of((uintptr_t)dst);
  if (bi >= 0 && !blocks[bi].live)
    return; /* (C1 has reported it) */
  if (!pitch)
    fill_run(dst, bytes, counts, poison);
  else
    for (size_t r = 0; r < rows; r++)
      fill_run((uint32_t *)((uint8_t *)dst + r * pitch), bytes, counts, poison);
}
static void fill_run(uint32_t *dst, size_t bytes, bool counts, uint32_t poison)
{
  if (poison || counts)
  {
    for (size_t i = 0; i < bytes / 4; i++)
      dst[i] = poison ? poison : sim_counts;
    if (poison)
      memset((uint8_t *)dst + (bytes & ~(size_t)3), 0xD0, bytes & 3);
  }
  else
    memset(dst, 0, bytes);
}
static void add_pending(Pending q)
{
  if (n_pend == room_pend)
    room_pend = room_pend ? 2 * room_pend : 256, pend = (Pending *)realloc(pend, room_pend * sizeof(Pending));
  pend[n_pend++] = q;
}
static int seen_depth;
static void seen(int s, uint64_t upto)
{
  seen_depth++;
  for (uint32_t i = 0; i < n_pend; i++)
  {
    Pending *q = &pend[i];
    if (!q->kind || q->stream != s || q->seq > upto)
      continue;
    const int bi = block_of((uintptr_t)q->p);
    if (q->kind == 'c' && bi >= 0 && blocks[bi].live && hash_bytes(q->p, q->n) != q->hash)
    {
      sim_violations++;
      printf("VIOLATION C5 the pinned input of %s (b%d+%zu, %zu bytes) was rewritten before the host saw it complete\n", q->name, bi,
             (size_t)((uintptr_t)q->p - blocks[bi].base), q->n);
    }
    if (q->kind == 'f')
      fill_words((uint32_t *)q->p, q->n, q->pitch, q->rows, q->counts, 0);
    q->kind = 0;
  }
  for (uint32_t i = 0; i < n_deps; i++)
    if (deps[i].stream == s && deps[i].at <= upto && deps[i].on >= 0)
    {
      const int on = deps[i].on;
      deps[i].on = -1;
      seen(on, deps[i].upto);
    }
  if (--seen_depth)
    return;
  uint32_t k = 0; /* compact */
  for (uint32_t i = 0; i < n_pend; i++)
    if (pend[i].kind)
      pend[k++] = pend[i];
  n_pend = k;
  k = 0;
  for (uint32_t i = 0; i < n_deps; i++)
    if (deps[i].on >= 0)
      deps[k++] = deps[i];
  n_deps = k;
}

static void complete_stream(int s, uint64_t upto)
{
  seen(s, upto);
  if (upto > streams[s].done_upto)
    streams[s].done_upto = upto;
  for (uint32_t i = 0; i < n_events; i++)
    if (events[i].stream == s && events[i].seq <= upto && events[i].cap == 0)
      events[i].busy = false;
}

int vksift_hip_event_record(vksift_hip_event e, vksift_hip_stream s)
{
  const int ei = event_id(e, "record of a dead event"), si = stream_id(s, "record on a dead stream");
  if (ei < 0 || si < 0)
    return 1;
  if (counted("event_record"))
    return SIM_ERR;
  Event *ev = &events[ei];
  ev->recorded = true, ev->stream = si, ev->seq = ++streams[si].seq, ev->cap = streams[si].cap;
  ev->busy = sim_busy_mode && ev->cap == 0;
  printf("#%llu rec e%d s%d%s\n", (unsigned long long)call_no, ei, si, ev->cap ? " captured" : "");
  return 0;
}
int vksift_hip_stream_wait_event(vksift_hip_stream s, vksift_hip_event e)
{
  const int ei = event_id(e, "wait on a dead event"), si = stream_id(s, "wait of a dead stream");
  if (ei < 0 || si < 0)
    return 1;
  if (counted("stream_wait_event"))
    return SIM_ERR;
  const Event *ev = &events[ei];
  printf("#%llu wait s%d e%d\n", (unsigned long long)call_no, si, ei);
  if (ev->cap && ev->cap == open_cap)
  {
    if (streams[si].cap == 0)
      streams[si].cap = open_cap, streams[si].joined_upto = streams[si].seq; /* joins the capture */
    if (ev->seq > streams[ev->stream].joined_upto)
      streams[ev->stream].joined_upto = ev->seq;
  }
  else if (ev->cap && streams[si].cap == 0)
    violation("C2", "a stream outside a capture waits on an event last recorded inside a finished capture: s, e", si, ei);
  else if (!ev->cap && streams[si].cap && ev->recorded && ev->busy)
    printf("note s%d (capturing) waits on e%d recorded outside the capture\n", si, ei);
  streams[si].seq++;
  if ((sim_roles || sim_late_posts) && sim_busy_mode && ev->recorded && ev->cap == 0 && streams[si].cap == 0)
  {
    if (n_deps == room_deps)
      room_deps = room_deps ? 2 * room_deps : 256, deps = (Dep *)realloc(deps, room_deps * sizeof(Dep));
    deps[n_deps++] = (Dep){si, ev->stream, streams[si].seq, ev->seq};
  }
  return 0;
}
int vksift_hip_stream_sync(vksift_hip_stream s)
{
  const int si = stream_id(s, "sync of a dead stream");
  if (si < 0)
    return 1;
  if (counted("stream_sync"))
    return SIM_ERR;
  printf("#%llu sync s%d\n", (unsigned long long)call_no, si);
  if (streams[si].cap)
    violation("C2", "stream_sync on a capturing stream", si, 0);
  streams[si].busy = false;
  complete_stream(si, streams[si].seq);
  return 0;
}
int vksift_hip_stream_busy(vksift_hip_stream s)
{
  const int si = stream_id(s, "query of a dead stream");
  if (si < 0)
    return -1;
  if (streams[si].cap)
    violation("C2", "stream_busy on a capturing stream", si, 0);
  return streams[si].busy ? 1 : 0;
}
static bool event_in_open_capture(int ei, const char *what)
{
  if (events[ei].cap && events[ei].cap == open_cap)
  {
    violation("C2", what, ei, 0);
    return true;
  }
  return false;
}
int vksift_hip_event_sync(vksift_hip_event e)
{
  const int ei = event_id(e, "sync of a dead event");
  if (ei < 0)
    return 1;
  if (counted("event_sync"))
    return SIM_ERR;
  printf("#%llu esync e%d\n", (unsigned long long)call_no, ei);
  if (!event_in_open_capture(ei, "event_sync on an event of the open capture") && events[ei].recorded && events[ei].cap == 0)
    complete_stream(events[ei].stream, events[ei].seq);
  return 0;
}
int vksift_hip_event_busy(vksift_hip_event e)
{
  const int ei = event_id(e, "query of a dead event");
  if (ei < 0)
    return -1;
  event_in_open_capture(ei, "event_busy on an event of the open capture");
  return events[ei].busy ? 1 : 0;
}
float vksift_hip_event_elapsed_ms(vksift_hip_event a, vksift_hip_event b)
{
  const int ai = event_id(a, "elapsed of a dead event"), bi = event_id(b, "elapsed of a dead event");
  if (ai >= 0 && bi >= 0)
    event_in_open_capture(ai, "event_elapsed_ms on an event of the open capture"), event_in_open_capture(bi, "event_elapsed_ms on an event of the open capture");
  return 1.0f;
}
void sim_drain(void)
{
  for (uint32_t i = 0; i < n_events; i++)
    events[i].busy = false;
  for (uint32_t i = 0; i < n_streams; i++)
    seen((int)i, streams[i].seq), streams[i].busy = false, streams[i].done_upto = streams[i].seq;
}

/* ------------------------------------------------------------------------------------------------ operations */
static Record cur;
static bool cur_open;

static void mix(const void *p, size_t n)
{
  const uint8_t *b = (const uint8_t *)p;
  for (size_t i = 0; i < n; i++)
    cur.digest = (cur.digest ^ b[i]) * 0x100000001b3ull;
}
static void mix_bound(const void *p, size_t n)
{
  const uint8_t *b = (const uint8_t *)p;
  for (size_t i = 0; i < n; i++)
    cur.bounds = (cur.bounds ^ b[i]) * 0x100000001b3ull;
}
static void note_block(int bi)
{
  for (uint32_t i = 0; i < cur.nblk; i++)
    if (cur.blk[i] == (uint32_t)bi)
      return;
  if (cur.nblk < MAX_REC_BLOCKS)
    cur.blk[cur.nblk++] = (uint32_t)bi;
  else
    violation("SIM", "more blocks in one operation than a record holds", bi, 0);
}
static void mix_ptr(uintptr_t v, int bi)
{
  const uint64_t w[2] = {0xb10cull << 32 | (uint32_t)bi, (uint64_t)(v - blocks[bi].base)};
  note_block(bi);
  mix(w, sizeof(w));
}
/* n bytes of argument: ledger pointers among its aligned words are normalised */
static void arg(const void *p, size_t n)
{
  const uint8_t *b = (const uint8_t *)p;
  size_t i = 0;
  for (; i + 8 <= n; i += 8)
  {
    uint64_t w;
    memcpy(&w, b + i, 8);
    const int bi = block_of((uintptr_t)w);
    if (bi >= 0)
      mix_ptr((uintptr_t)w, bi);
    else
      mix(&w, 8);
  }
  mix(b + i, n - i);
}
/* a pointer argument: a ledger address, NULL, or host memory of `bytes` bytes (0: unknown length, a tag) */
static void arg_arr(const void *p, size_t bytes)
{
  const int bi = block_of((uintptr_t)p);
  if (bi >= 0)
    mix_ptr((uintptr_t)p, bi);
  else if (!p)
    mix("null", 4);
  else if (bytes)
    arg(p, bytes);
  else
    mix("host", 4);
}
static void arg_plane(const vksift_hip_Plane *p)
{
  arg_arr(p->base, 0);
  mix(&p->w, 4), mix(&p->h, 4), mix(&p->pitch, 4), mix(&p->img_stride, 8), mix(&p->fp16, 4), mix(&p->reverse, 4);
}
static void arg_planes(const vksift_hip_Plane *p, uint32_t n)
{
  for (uint32_t i = 0; i < n; i++)
    arg_plane(&p[i]);
}

/* the roles of the operation being recorded (sim_roles): the text of its "args" line, and the pinned inputs to hash (C5) */
static char roles[2048];
static size_t roles_n;
static struct
{
  const void *p;
  size_t n;
} pinned_in[8];
static uint32_t n_pinned_in;
static bool cur_late; /* its effect is a posting or a device-to-host copy (sim_late_posts) */

/* a pointer argument of a role-known operation: digested as P() digests it; role 'r' / 'w', `bytes` it may touch (0: not stated) */
static void arg_role(const char *arg_name, const void *p, size_t bytes, char role)
{
  arg_arr(p, 0);
  if (!sim_roles)
    return;
  const int bi = block_of((uintptr_t)p);
  if (bi < 0)
  {
    roles_n += (size_t)snprintf(roles + roles_n, sizeof(roles) - roles_n, " %s=-:%c:%zu", arg_name, role, bytes);
    return;
  }
  const size_t off = (size_t)((uintptr_t)p - blocks[bi].base);
  roles_n += (size_t)snprintf(roles + roles_n, sizeof(roles) - roles_n, " %s=b%d+%zu:%c:%zu", arg_name, bi, off, role, bytes);
  if (roles_n >= sizeof(roles))
    roles_n = sizeof(roles) - 1;
  if (off + bytes > blocks[bi].bytes)
  {
    sim_violations++;
    printf("VIOLATION C4 %s %s: %zu bytes from offset %zu of b%d, which holds %zu\n", cur.name, arg_name, bytes, off, bi, blocks[bi].bytes);
  }
  else if (role == 'r' && bytes && blocks[bi].kind == 'H' && blocks[bi].live && sim_busy_mode && n_pinned_in < 8)
    pinned_in[n_pinned_in].p = p, pinned_in[n_pinned_in++].n = bytes;
}
/* C4, the other half: with more than one slot, what a slot may hold (max_n x element) fits its stride — what the launchers themselves refuse */
static void slot_fits(const char *what, uint64_t per_slot, uint64_t stride, uint32_t nslots)
{
  if (sim_roles && nslots > 1 && per_slot > stride)
  {
    sim_violations++;
    printf("VIOLATION C4 %s %s: a slot may hold %llu bytes, its stride is %llu\n", cur.name, what, (unsigned long long)per_slot, (unsigned long long)stride);
  }
}
#define FITS(x, per_slot, stride) slot_fits(#x, (uint64_t)(per_slot), (uint64_t)(stride), nslots)
#define RD(x, bytes) arg_role(#x, x, (size_t)(bytes), 'r')
#define WR(x, bytes) arg_role(#x, x, (size_t)(bytes), 'w')
/* words of a strided single-word (or `k`-word) read per slot: the last slot's words end it */
#define STRIDED(nslots, stride, k) ((nslots) ? (((size_t)(nslots) - 1u) * (size_t)(stride) + (size_t)(k)) * 4u : 0u)

static bool op_begin(const char *name, vksift_hip_stream s)
{
  const int si = stream_id(s, name);
  memset(&cur, 0, sizeof(cur));
  roles_n = 0, roles[0] = 0, n_pinned_in = 0, cur_late = false;
  if (counted(name))
    return true;
  snprintf(cur.name, sizeof(cur.name), "%s", name);
  cur.stream = si, cur.digest = 0xcbf29ce484222325ull;
  cur_open = true;
  return false;
}
static void run_effect(const Record *r)
{
  if (!r->fill)
    return;
  const int bi = block_of((uintptr_t)r->fill);
  if (bi >= 0 && !blocks[bi].live)
    return; /* (C1 has reported it) */
  if (r->fill_pitch)
    fill_words(r->fill, r->fill_bytes, r->fill_pitch, r->fill_rows, r->fill_counts, 0);
  else if (r->fill_counts)
    for (size_t i = 0; i < r->fill_bytes / 4; i++)
      r->fill[i] = sim_counts;
  else
    memset(r->fill, 0, r->fill_bytes);
}
static void check_live(const Record *r, const char *how)
{
  for (uint32_t i = 0; i < r->nblk; i++)
    if (!blocks[r->blk[i]].live)
    {
      printf("VIOLATION C1 %s %s names the dead block b%u\n", how, r->name, r->blk[i]);
      sim_violations++;
    }
}
static int op_end(void)
{
  cur_open = false;
  if (cur.stream < 0)
    return 1;
  Stream *st = &streams[cur.stream];
  st->seq++;
  check_live(&cur, st->cap ? "captured" : "issued");
  if (st->cap)
  {
    if (cap_n == cap_room)
    {
      cap_room = cap_room ? 2 * cap_room : 256;
      cap_recs = (Record *)realloc(cap_recs, cap_room * sizeof(Record));
    }
    cap_recs[cap_n++] = cur;
    printf("#%llu cop %s s%d %016llx %016llx\n", (unsigned long long)call_no, cur.name, cur.stream, (unsigned long long)cur.digest, (unsigned long long)cur.bounds);
    return 0;
  }
  st->busy = sim_busy_mode != 0;
  printf("#%llu op %s s%d %016llx %016llx\n", (unsigned long long)call_no, cur.name, cur.stream, (unsigned long long)cur.digest, (unsigned long long)cur.bounds);
  if (sim_roles && roles_n)
    printf("args %s%s\n", cur.name, roles);
  for (uint32_t i = 0; i < n_pinned_in; i++)
  {
    Pending q = {cur.stream, st->seq, 'c', (void *)(uintptr_t)pinned_in[i].p, pinned_in[i].n, hash_bytes(pinned_in[i].p, pinned_in[i].n), false, "", 0, 0};
    memcpy(q.name, cur.name, sizeof(q.name));
    add_pending(q);
  }
  if (cur_late && cur.fill && sim_late_posts && sim_busy_mode)
  {
    Pending q = {cur.stream, st->seq, 'f', cur.fill, cur.fill_bytes, 0, cur.fill_counts, "", cur.fill_pitch, cur.fill_rows};
    const int bi = block_of((uintptr_t)cur.fill);
    if (bi < 0 || blocks[bi].live)
      fill_words(cur.fill, cur.fill_bytes, cur.fill_pitch, cur.fill_rows, false, SIM_POISON), add_pending(q);
    return 0;
  }
  run_effect(&cur);
  return 0;
}
#define OP(name, s)       \
  if (op_begin(name, s)) \
  return SIM_ERR
#define OPT(name, s) \
  if (!sim_covered)  \
    return -1;       \
  OP(name, s)
#define V(x) arg(&(x), sizeof(x))
#define T(x) mix_bound(&(x), sizeof(x))
#define P(x) arg_arr(x, 0)
#define A(p, bytes) arg_arr(p, bytes)
#define END return op_end()

/* ------------------------------------------------------------------------------------------------ capture and graphs */
int vksift_hip_capture_begin(vksift_hip_stream s)
{
  const int si = stream_id(s, "capture_begin on a dead stream");
  if (si < 0)
    return 1;
  if (counted("capture_begin"))
    return SIM_ERR;
  if (open_cap)
    violation("C2", "capture_begin with a capture open", si, open_cap);
  open_cap = ++n_caps, open_origin = si, cap_invalid = false;
  streams[si].cap = open_cap;
  cap_n = 0;
  printf("#%llu capbegin s%d\n", (unsigned long long)call_no, si);
  return 0;
}
int vksift_hip_capture_end(vksift_hip_stream s, vksift_hip_graph *out)
{
  const int si = stream_id(s, "capture_end on a dead stream");
  *out = NULL;
  if (si < 0)
    return 1;
  const bool fail = counted("capture_end") || cap_invalid;
  if (!open_cap || open_origin != si)
  {
    violation("C2", "capture_end on a stream that is not a capture's origin", si, open_cap);
    return 1;
  }
  for (uint32_t i = 0; i < n_streams; i++)
  {
    if (streams[i].cap == open_cap && (int)i != si && streams[i].seq > streams[i].joined_upto && !fail)
      violation("C2", "capture_end with a joined stream that has not rejoined the origin", (long)i, 0);
    if (streams[i].cap == open_cap)
      streams[i].cap = 0;
  }
  open_cap = 0, open_origin = -1; /* (a failed end invalidates the capture: it is closed either way) */
  if (fail || n_execs == MAX_EXECS)
  {
    printf("capend s%d invalid\n", si);
    return SIM_ERR;
  }
  Exec *x = &execs[n_execs++];
  x->live = true, x->destroyed = false, x->n = cap_n, x->last_stream = -1;
  x->recs = (Record *)malloc((cap_n ? cap_n : 1) * sizeof(Record));
  memcpy(x->recs, cap_recs, cap_n * sizeof(Record));
  printf("#%llu capend s%d x%ld n=%u\n", (unsigned long long)call_no, si, (long)(x - execs), cap_n);
  *out = x;
  return 0;
}
static Exec *exec_of(vksift_hip_graph g, const char *who)
{
  Exec *x = (Exec *)g;
  if ((uintptr_t)g < (uintptr_t)execs || x - execs >= (long)n_execs)
  {
    violation("C3", who, -1, 0);
    return NULL;
  }
  if (x->destroyed)
  {
    violation("C3", who, (long)(x - execs), 0);
    return NULL;
  }
  return x;
}
int vksift_hip_graph_launch(vksift_hip_graph g, vksift_hip_stream s)
{
  const int si = stream_id(s, "graph_launch on a dead stream");
  Exec *x = exec_of(g, "launch of a destroyed exec");
  if (si < 0 || !x)
    return 1;
  if (counted("graph_launch"))
    return SIM_ERR;
  printf("#%llu launch x%ld s%d\n", (unsigned long long)call_no, (long)(x - execs), si);
  if (streams[si].cap)
    violation("C2", "graph_launch into a capturing stream", si, 0);
  streams[si].seq++;
  streams[si].busy = sim_busy_mode != 0;
  x->last_stream = sim_busy_mode ? si : -1, x->last_seq = streams[si].seq;
  for (uint32_t i = 0; i < x->n; i++)
  {
    check_live(&x->recs[i], "replayed");
    printf("gop %s s%d %016llx %016llx\n", x->recs[i].name, x->recs[i].stream, (unsigned long long)x->recs[i].digest, (unsigned long long)x->recs[i].bounds);
    run_effect(&x->recs[i]);
  }
  return 0;
}
void vksift_hip_graph_destroy(vksift_hip_graph g)
{
  if (!g)
    return;
  Exec *x = exec_of(g, "destruction of a destroyed exec");
  if (!x)
    return;
  printf("xdestroy x%ld\n", (long)(x - execs));
  if (x->last_stream >= 0 && streams[x->last_stream].live && x->last_seq > streams[x->last_stream].done_upto)
    violation("C3", "an exec is destroyed while its last launch may still be executing: exec, stream", (long)(x - execs), x->last_stream);
  x->destroyed = true, x->live = false;
  free(x->recs);
  x->recs = NULL;
}

/* C2, last clause: the harness calls this behind every API call */
void sim_api_return(void)
{
  if (open_cap)
  {
    violation("C2", "a capture is open when the API call returns", open_origin, open_cap);
    for (uint32_t i = 0; i < n_streams; i++)
      streams[i].cap = 0;
    open_cap = 0, open_origin = -1;
  }
  if (range_depth)
  {
    sim_violations++;
    printf("VIOLATION C2 %d profiler ranges are open when the API call returns\n", range_depth);
    range_depth = 0;
  }
  for (uint32_t i = 0; i < n_pend; i++) /* caller memory does not outlive the call: a copy into it that nothing waited for never arrives */
    if (pend[i].kind == 'f' && block_of((uintptr_t)pend[i].p) < 0)
      pend[i].kind = 0;
}
/* C3: what is still live */
void sim_report_ledger(void)
{
  uint32_t lb = 0, ls = 0, le = 0, lx = 0;
  for (uint32_t i = 0; i < n_blocks; i++)
    lb += blocks[i].live;
  for (uint32_t i = 0; i < n_streams; i++)
    ls += streams[i].live;
  for (uint32_t i = 0; i < n_events; i++)
    le += events[i].live;
  for (uint32_t i = 0; i < n_execs; i++)
    lx += execs[i].live;
  printf("ledger blocks=%u streams=%u events=%u execs=%u violations=%llu\n", lb, ls, le, lx, (unsigned long long)sim_violations);
}
uint32_t sim_live_execs(void)
{
  uint32_t lx = 0;
  for (uint32_t i = 0; i < n_execs; i++)
    lx += execs[i].live;
  return lx;
}
/* the end of the process: the host memory the simulation itself holds */
void sim_finish(void)
{
  for (uint32_t i = 0; i < n_blocks; i++)
    if (blocks[i].kind == 'H')
    {
      UNPOISON((void *)blocks[i].base, blocks[i].bytes ? blocks[i].bytes : 1);
      free((void *)blocks[i].base);
    }
  for (uint32_t i = 0; i < n_execs; i++)
    free(execs[i].recs);
  free(cap_recs);
  free(pend), free(deps);
  pend = NULL, deps = NULL, n_pend = room_pend = n_deps = room_deps = 0;
  cap_recs = NULL, cap_room = cap_n = 0;
  n_blocks = 0;
}

/* ------------------------------------------------------------------------------------------------ copies */
int vksift_hip_memcpy_h2d(void *dst, const void *src, size_t n, vksift_hip_stream s)
{
  OP("memcpy_h2d", s);
  WR(dst, n), RD(src, n), V(n);
  END;
}
int vksift_hip_memcpy_d2h(void *dst, const void *src, size_t n, vksift_hip_stream s)
{
  OP("memcpy_d2h", s);
  WR(dst, n), RD(src, n), V(n);
  cur_late = true;
  cur.fill = (uint32_t *)dst, cur.fill_bytes = n, cur.fill_counts = false;
  END;
}
int vksift_hip_memcpy_d2d(void *dst, const void *src, size_t n, vksift_hip_stream s)
{
  OP("memcpy_d2d", s);
  WR(dst, n), RD(src, n), V(n);
  END;
}
int vksift_hip_memcpy2d_d2h(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t height, vksift_hip_stream s)
{
  OP("memcpy2d_d2h", s);
  WR(dst, height ? (height - 1u) * dpitch + width_bytes : 0u), V(dpitch), RD(src, height ? (height - 1u) * spitch + width_bytes : 0u), V(spitch), V(width_bytes), V(height);
  cur_late = true;
  if (dpitch == width_bytes)
    cur.fill = (uint32_t *)dst, cur.fill_bytes = width_bytes * height, cur.fill_counts = false;
  else if (sim_late_posts) /* (row by row, the gaps untouched; without the switch a pitched copy leaves its destination as it is, as it always did) */
    cur.fill = (uint32_t *)dst, cur.fill_bytes = width_bytes, cur.fill_pitch = dpitch, cur.fill_rows = height, cur.fill_counts = false;
  END;
}
int vksift_hip_post_words(uint32_t *host_mapped_dst, const uint32_t *src, size_t n_words, vksift_hip_stream s)
{
  OP("post_words", s);
  WR(host_mapped_dst, 4u * n_words), RD(src, 4u * n_words), V(n_words);
  cur_late = true;
  cur.fill = host_mapped_dst, cur.fill_bytes = 4 * n_words, cur.fill_counts = true;
  END;
}
int vksift_hip_memset(void *dst, int value, size_t n, vksift_hip_stream s)
{
  OP("memset", s);
  WR(dst, n), V(value), V(n);
  END;
}

/* ------------------------------------------------------------------------------------------------ pyramid */
int vksift_hip_input_blit(const uint8_t *src, uint32_t sw, uint32_t sh, uint64_t src_img_stride, vksift_hip_Plane dst, uint32_t batch, vksift_hip_stream s)
{
  OP("input_blit", s);
  P(src), V(sw), V(sh), V(src_img_stride), arg_plane(&dst), V(batch);
  END;
}
int vksift_hip_blur(vksift_hip_Plane src, vksift_hip_Plane dst, const float *taps, uint32_t ntaps, uint32_t batch, vksift_hip_stream s)
{
  OP("blur", s);
  arg_plane(&src), arg_plane(&dst), A(taps, 4u * ntaps), V(ntaps), V(batch);
  END;
}
int vksift_hip_blur_pair(vksift_hip_Plane src, vksift_hip_Plane dst1, vksift_hip_Plane dst2, const float *taps1, uint32_t ntaps1, const float *taps2, uint32_t ntaps2,
                         uint32_t batch, vksift_hip_stream s)
{
  OPT("blur_pair", s);
  arg_plane(&src), arg_plane(&dst1), arg_plane(&dst2), A(taps1, 4u * ntaps1), V(ntaps1), A(taps2, 4u * ntaps2), V(ntaps2), V(batch);
  END;
}
int vksift_hip_blur_multi(const vksift_hip_Plane *src, const vksift_hip_Plane *dst, uint32_t n, const float *taps, uint32_t ntaps, uint32_t batch, vksift_hip_stream s)
{
  OPT("blur_multi", s);
  arg_planes(src, n), arg_planes(dst, n), V(n), A(taps, 4u * ntaps), V(ntaps), V(batch);
  END;
}
int vksift_hip_blur_downsample(vksift_hip_Plane src, vksift_hip_Plane dst, vksift_hip_Plane next, const float *taps, uint32_t ntaps, uint32_t batch, vksift_hip_stream s)
{
  OPT("blur_downsample", s);
  arg_plane(&src), arg_plane(&dst), arg_plane(&next), A(taps, 4u * ntaps), V(ntaps), V(batch);
  END;
}
int vksift_hip_seed_upsampled(const uint8_t *src, uint32_t sw, uint32_t sh, uint64_t src_img_stride, vksift_hip_Plane dst, const float *taps, uint32_t ntaps, uint32_t batch,
                              vksift_hip_stream s)
{
  OPT("seed_upsampled", s);
  P(src), V(sw), V(sh), V(src_img_stride), arg_plane(&dst), A(taps, 4u * ntaps), V(ntaps), V(batch);
  END;
}
int vksift_hip_seed_direct(const uint8_t *src, uint32_t sw, uint32_t sh, uint64_t src_img_stride, vksift_hip_Plane dst, const float *taps, uint32_t ntaps, uint32_t batch,
                           vksift_hip_stream s)
{
  OPT("seed_direct", s);
  P(src), V(sw), V(sh), V(src_img_stride), arg_plane(&dst), A(taps, 4u * ntaps), V(ntaps), V(batch);
  END;
}
int vksift_hip_downsample(vksift_hip_Plane src, vksift_hip_Plane dst, uint32_t batch, vksift_hip_stream s)
{
  OP("downsample", s);
  arg_plane(&src), arg_plane(&dst), V(batch);
  END;
}
int vksift_hip_octave_chain(const vksift_hip_Plane *layers, uint32_t n_oct, uint32_t n_layers, uint32_t S, const float *taps, const uint32_t *ntaps, uint32_t batch,
                            vksift_hip_stream s)
{
  if (S >= n_layers) /* the host's test hook: outside the launcher's domain, it declines */
    return -1;
  OPT("octave_chain", s);
  arg_planes(layers, n_oct * n_layers), V(n_oct), V(n_layers), V(S), A(taps, 4u * VKSIFT_HIP_MAX_TAPS * n_layers), A(ntaps, 4u * n_layers), V(batch);
  END;
}
int vksift_hip_dog_plane(const float *lo, const float *hi, uint32_t w, uint32_t h, uint32_t pitch, uint32_t fp16, float *out_dense, vksift_hip_stream s)
{
  OP("dog_plane", s);
  P(lo), P(hi), V(w), V(h), V(pitch), V(fp16), P(out_dense);
  END;
}

/* ------------------------------------------------------------------------------------------------ keypoints */
static void arg_jobs(const vksift_hip_OctaveJob *jobs, uint32_t n)
{
  for (uint32_t i = 0; i < n; i++)
  {
    vksift_hip_OctaveJob j = jobs[i];
    arg(&j, sizeof(j));
  }
}
int vksift_hip_extract_keypoints_multi(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s, vksift_hip_event scan_done)
{
  OP("extract_keypoints_multi", s);
  arg_jobs(jobs, n_jobs), V(n_jobs), V(batch);
  const int e = op_end();
  if (e == 0 && scan_done)
    return vksift_hip_event_record(scan_done, s);
  return e;
}
int vksift_hip_clear_segment_masks(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s)
{
  OPT("clear_segment_masks", s);
  arg_jobs(jobs, n_jobs), V(n_jobs), V(batch);
  END;
}
int vksift_hip_orientations_multi(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s)
{
  OP("orientations_multi", s);
  arg_jobs(jobs, n_jobs), V(n_jobs), V(batch);
  END;
}
int vksift_hip_descriptors_multi(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s)
{
  OP("descriptors_multi", s);
  arg_jobs(jobs, n_jobs), V(n_jobs), V(batch);
  END;
}
int vksift_hip_descriptors_multi_dense(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, const vksift_hip_DenseRows *dense, vksift_hip_stream s)
{
  OP("descriptors_multi_dense", s);
  arg_jobs(jobs, n_jobs), V(n_jobs), V(batch);
  if (dense)
  {
    vksift_hip_DenseRows d = *dense;
    arg(&d, sizeof(d));
    if (d.found_post) /* feature posting: the counters reach the host through this launch */
      cur.fill = d.found_post, cur.fill_bytes = 4u * d.found_post_n, cur.fill_counts = true;
  }
  END;
}
int vksift_hip_place_keypoints(const vksift_hip_Keypoint *kps, const uint32_t *kp_first, const vksift_hip_PlaceOctave *oct, uint32_t n_oct, const float *sigma_steps,
                               uint32_t S, uint32_t keep_orientation, uint32_t batch, uint32_t *placed, vksift_hip_stream s)
{
  OP("place_keypoints", s);
  P(kps), P(kp_first);
  for (uint32_t o = 0; o < n_oct; o++)
  {
    const vksift_hip_PlaceOctave *q = &oct[o];
    V(q->w), V(q->h), V(q->octave_idx), P(q->feats), V(q->feat_img_stride), V(q->cap), P(q->found), V(q->found_img_stride);
  }
  V(n_oct), A(sigma_steps, 4u * (S + 1u)), V(S), V(keep_orientation), V(batch), P(placed);
  END;
}

/* ------------------------------------------------------------------------------------------------ records and matcher */
int vksift_hip_shifted_norms(const uint8_t *desc, uint32_t n, uint32_t *norms, vksift_hip_stream s)
{
  OP("shifted_norms", s);
  P(desc), V(n), P(norms);
  END;
}
int vksift_hip_match_2nn_prenormed(const uint8_t *desc_a, const uint32_t *norm_a, uint32_t na, uint32_t a_index_base, const uint8_t *desc_b, const uint32_t *norm_b,
                                   uint32_t nb, uint32_t *scratch, size_t scratch_u32, uint8_t *matches, vksift_hip_stream s)
{
  OP("match_2nn_prenormed", s);
  P(desc_a), P(norm_a), V(na), V(a_index_base), P(desc_b), P(norm_b), V(nb), P(scratch), V(scratch_u32), P(matches);
  END;
}
int vksift_hip_filter_matches(const uint8_t *fwd, uint64_t fwd_slot_stride, const uint8_t *rev, uint64_t rev_slot_stride, const uint32_t *n_fwd, uint32_t n_stride,
                              float ratio, uint32_t nslots, uint8_t *out, uint64_t out_slot_stride, uint32_t *out_n, vksift_hip_stream s)
{
  OP("filter_matches", s);
  RD(fwd, fwd_slot_stride * nslots), V(fwd_slot_stride), RD(rev, rev ? rev_slot_stride * nslots : 0u), V(rev_slot_stride), RD(n_fwd, STRIDED(nslots, n_stride, 2)), V(n_stride),
      V(ratio), V(nslots), WR(out, out_slot_stride * nslots), V(out_slot_stride), WR(out_n, 4u * nslots);
  END;
}
int vksift_hip_pack_features(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, const uint32_t *out_rows, uint32_t nslots, uint32_t nsec,
                             const uint32_t *sec_off, const uint32_t *sec_cap, const uint32_t *found_base, uint32_t found_buf_stride, uint8_t *out, uint32_t max_rows,
                             uint32_t *found_post, vksift_hip_stream s)
{
  OP("pack_features", s);
  RD(feats_base, 0), V(buf_stride), A(buf_ids, 4u * nslots), A(out_rows, 4u * nslots), V(nslots), V(nsec), A(sec_off, 4u * nsec), A(sec_cap, 4u * nsec), RD(found_base, 0),
      V(found_buf_stride), WR(out, 0), T(max_rows), WR(found_post, 0);
  END;
}
/* (the records and cache entries are addressed by buffer id: the header states no extent in the launch's own scalars. FEATS / FOUND: the role of the two) */
#define SECTION_ARGS(FEATS, FOUND)                                                                                                                                 \
  FEATS(feats_base, 0), V(buf_stride), A(buf_ids, 4u * nslots), V(nslots), V(nsec), A(sec_off, 4u * nsec), A(sec_cap, 4u * nsec), A(fixed_counts, 4u * nsec), FOUND(found_base, 0), \
      V(found_buf_stride)
#define CACHE_ARGS V(pad_rows_to), WR(desc, 0), V(desc_stride), WR(norms, 0), V(norm_stride), WR(n_out_dev, 0), V(n_stride)
int vksift_hip_gather_sections(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec, const uint32_t *sec_off,
                               const uint32_t *sec_cap, const uint32_t *fixed_counts, const uint32_t *found_base, uint32_t found_buf_stride, uint32_t max_rows,
                               uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_stride, uint32_t *norms, uint64_t norm_stride, uint32_t *n_out_dev, uint32_t n_stride,
                               vksift_hip_stream s)
{
  OP("gather_sections", s);
  SECTION_ARGS(RD, RD), T(max_rows), CACHE_ARGS;
  END;
}
int vksift_hip_keep_strongest(uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec, const uint32_t *sec_off,
                              const uint32_t *sec_cap, const uint32_t *fixed_counts, uint32_t *found_base, uint32_t found_buf_stride, uint32_t *found_post,
                              uint32_t max_features, uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_stride, uint32_t *norms, uint64_t norm_stride, uint32_t *n_out_dev,
                              uint32_t n_stride, vksift_hip_stream s)
{
  OP("keep_strongest", s);
  SECTION_ARGS(WR, WR), WR(found_post, 0), V(max_features), CACHE_ARGS;
  END;
}
int vksift_hip_keep_grid(uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec, const uint32_t *sec_off, const uint32_t *sec_cap,
                         const uint32_t *fixed_counts, uint32_t *found_base, uint32_t found_buf_stride, uint32_t *found_post, uint32_t max_features, uint32_t grid_cols,
                         uint32_t grid_rows, const float *col_bounds, const float *row_bounds, uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_stride, uint32_t *norms,
                         uint64_t norm_stride, uint32_t *n_out_dev, uint32_t n_stride, vksift_hip_stream s)
{
  OP("keep_grid", s);
  SECTION_ARGS(WR, WR), WR(found_post, 0), V(max_features), V(grid_cols), V(grid_rows), A(col_bounds, grid_cols ? 4u * (grid_cols - 1u) : 0u),
      A(row_bounds, grid_rows ? 4u * (grid_rows - 1u) : 0u), CACHE_ARGS;
  END;
}
int vksift_hip_root_descriptors(uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec, const uint32_t *sec_off,
                                const uint32_t *sec_cap, const uint32_t *fixed_counts, const uint32_t *found_base, uint32_t found_buf_stride, uint32_t max_rows,
                                uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_stride, uint32_t *norms, uint64_t norm_stride, uint32_t *n_out_dev, uint32_t n_stride,
                                vksift_hip_stream s)
{
  OP("root_descriptors", s);
  SECTION_ARGS(WR, RD), T(max_rows), CACHE_ARGS;
  END;
}
int vksift_hip_match_2nn_async(const uint8_t *cache_desc, const uint32_t *cache_norm, const uint32_t *cache_n, const uint32_t *ids_a, const uint32_t *ids_b, uint32_t max_na,
                               uint32_t max_nb, uint32_t nb_exact, uint32_t *redo, uint32_t *n_dev, uint8_t *matches, uint32_t nslots, uint64_t cache_desc_stride,
                               uint64_t cache_norm_stride, uint64_t redo_slot_stride, uint64_t match_slot_stride, uint32_t n_slot_stride, uint32_t *partial_scratch,
                               vksift_hip_stream s)
{
  OP("match_2nn_async", s);
  RD(cache_desc, 0), RD(cache_norm, 0), RD(cache_n, 0), A(ids_a, 4u * nslots), A(ids_b, 4u * nslots), T(max_na), T(max_nb), T(nb_exact), WR(redo, 4u * redo_slot_stride * nslots),
      WR(n_dev, STRIDED(nslots, n_slot_stride, 2)), WR(matches, match_slot_stride * nslots), V(nslots), V(cache_desc_stride), V(cache_norm_stride), V(redo_slot_stride),
      V(match_slot_stride), V(n_slot_stride), WR(partial_scratch, partial_scratch ? (size_t)20u * max_na * VKSIFT_HIP_MATCH_CHUNKS : 0u);
  END;
}

/* ------------------------------------------------------------------------------------------------ the stages behind a filtered matching */
/* a pair table's layouts: at most one per buffer, two buffers per slot, 33 words each (include/vksift_hip.h) */
#define LAYOUT_BYTES(nslots) ((size_t)2u * (nslots) * 33u * 4u)
int vksift_hip_gather_correspondences(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *found_base, uint32_t found_buf_stride, const uint32_t *slot_tab,
                                      const uint32_t *layouts, const uint8_t *filtered, uint64_t filtered_slot_stride, const uint32_t *filtered_n, uint32_t max_n,
                                      uint32_t nslots, float *corr, uint64_t corr_slot_stride, vksift_hip_stream s)
{
  OP("gather_correspondences", s);
  RD(feats_base, 0), V(buf_stride), RD(found_base, 0), V(found_buf_stride), RD(slot_tab, 16u * nslots), RD(layouts, LAYOUT_BYTES(nslots)), RD(filtered, filtered_slot_stride * nslots),
      V(filtered_slot_stride), RD(filtered_n, 4u * nslots), V(max_n), V(nslots), WR(corr, corr_slot_stride * nslots), V(corr_slot_stride),
      FITS(corr, 16u * (uint64_t)max_n, corr_slot_stride), FITS(filtered, 16u * (uint64_t)max_n, filtered_slot_stride);
  END;
}
#define RANSAC_ARGS                                                                                                                                                \
  RD(corr, corr_slot_stride * nslots), V(corr_slot_stride), RD(n_dev, STRIDED(nslots, n_stride, 1)), V(n_stride), V(max_n), V(nslots), V(nb_hypotheses), V(threshold_px), V(seed), \
      WR(results, (size_t)RES_BYTES * nslots), WR(masks, mask_slot_stride * nslots), V(mask_slot_stride), WR(scratch, 4u * scratch_u32), V(scratch_u32),      \
      FITS(corr, 16u * (uint64_t)max_n, corr_slot_stride), FITS(masks, max_n, mask_slot_stride)
int vksift_hip_ransac_homography(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                 uint32_t nb_hypotheses, float threshold_px, uint64_t seed, uint8_t *results, uint8_t *masks, uint64_t mask_slot_stride, uint32_t *scratch,
                                 size_t scratch_u32, vksift_hip_stream s)
{
  OP("ransac_homography", s);
  enum { RES_BYTES = 52 };
  RANSAC_ARGS;
  END;
}
int vksift_hip_ransac_fundamental(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                  uint32_t nb_hypotheses, float threshold_px, uint64_t seed, uint8_t *results, uint8_t *masks, uint64_t mask_slot_stride, uint32_t *scratch,
                                  size_t scratch_u32, vksift_hip_stream s)
{
  OP("ransac_fundamental", s);
  enum { RES_BYTES = 56 };
  RANSAC_ARGS;
  END;
}
#define REFIT_ARGS                                                                                                                                                 \
  RD(corr, corr_slot_stride * nslots), V(corr_slot_stride), RD(n_dev, STRIDED(nslots, n_stride, 1)), V(n_stride), V(max_n), V(nslots), RD(start_results, (size_t)START_BYTES * nslots), \
      RD(start_masks, mask_slot_stride * nslots), V(mask_slot_stride), V(nb_rounds), V(threshold_px), WR(results, (size_t)52u * nslots), WR(masks_out, mask_slot_stride * nslots), \
      FITS(corr, 16u * (uint64_t)max_n, corr_slot_stride), FITS(masks_out, max_n, mask_slot_stride)
int vksift_hip_refit_homography(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                const uint8_t *start_results, const uint8_t *start_masks, uint64_t mask_slot_stride, uint32_t nb_rounds, float threshold_px,
                                uint8_t *results, uint8_t *masks_out, vksift_hip_stream s)
{
  OP("refit_homography", s);
  enum { START_BYTES = 52 };
  REFIT_ARGS;
  END;
}
int vksift_hip_refit_fundamental(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                 const uint8_t *start_results, const uint8_t *start_masks, uint64_t mask_slot_stride, uint32_t nb_rounds, float threshold_px,
                                 uint8_t *results, uint8_t *masks_out, vksift_hip_stream s)
{
  OP("refit_fundamental", s);
  enum { START_BYTES = 56 };
  REFIT_ARGS;
  END;
}
int vksift_hip_gather_xy(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *found_base, uint32_t found_buf_stride, const uint32_t *slot_tab,
                         const uint32_t *layouts, uint32_t max_n, uint32_t nslots, float *xy, uint64_t xy_side_stride, vksift_hip_stream s)
{
  OP("gather_xy", s);
  RD(feats_base, 0), V(buf_stride), RD(found_base, 0), V(found_buf_stride), RD(slot_tab, 16u * nslots), RD(layouts, LAYOUT_BYTES(nslots)), V(max_n), V(nslots),
      WR(xy, (size_t)2u * nslots * xy_side_stride * 8u), V(xy_side_stride), FITS(xy, max_n, xy_side_stride);
  END;
}
int vksift_hip_match_guided(const uint8_t *cache_desc, uint64_t cache_desc_stride, const uint32_t *cache_norm, uint64_t cache_norm_stride, const uint32_t *slot_tab,
                            uint32_t slot_tab_stride, const float *xy, uint64_t xy_side_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, const float *models,
                            uint32_t model_stride, const uint32_t *valid, uint32_t valid_stride, uint32_t model_kind, float t2, float ratio, float max_distance,
                            uint32_t cross_check, uint32_t nslots, uint8_t *out, uint64_t out_slot_stride, uint32_t *out_n, uint32_t *scratch, size_t scratch_u32,
                            vksift_hip_stream s)
{
  OP("match_guided", s);
  RD(cache_desc, 0), V(cache_desc_stride), RD(cache_norm, 0), V(cache_norm_stride), RD(slot_tab, STRIDED(nslots, slot_tab_stride, 2)), V(slot_tab_stride),
      RD(xy, (size_t)2u * nslots * xy_side_stride * 8u), V(xy_side_stride), RD(n_dev, STRIDED(nslots, n_stride, 2)), V(n_stride), V(max_n), RD(models, STRIDED(nslots, model_stride, 9)),
      V(model_stride), RD(valid, STRIDED(nslots, valid_stride, 1)), V(valid_stride), V(model_kind), V(t2), V(ratio), V(max_distance), V(cross_check), V(nslots),
      WR(out, out_slot_stride * nslots), V(out_slot_stride), WR(out_n, 4u * nslots), WR(scratch, 4u * scratch_u32), V(scratch_u32), FITS(out, 16u * (uint64_t)max_n, out_slot_stride),
      FITS(xy, max_n, xy_side_stride), FITS(cache_desc, 128u * (uint64_t)max_n, cache_desc_stride), FITS(cache_norm, max_n, cache_norm_stride);
  END;
}

/* ------------------------------------------------------------------------------------------------ feature tracks */
int vksift_hip_build_tracks(const uint8_t *records, uint64_t rec_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, const uint8_t *masks,
                            uint64_t mask_slot_stride, const uint32_t *valid, uint32_t valid_stride, const uint32_t *slot_tab, uint32_t slot_tab_stride, uint32_t nslots,
                            const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, uint32_t *node_words,
                            uint8_t *tracks, uint64_t tracks_cap, uint32_t *stats, uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s)
{
  OP("build_tracks", s);
  RD(records, rec_slot_stride * nslots), V(rec_slot_stride), RD(n_dev, STRIDED(nslots, n_stride, 1)), V(n_stride), V(max_n), RD(masks, masks ? mask_slot_stride * nslots : 0u),
      V(mask_slot_stride), RD(valid, valid ? STRIDED(nslots, valid_stride, 1) : 0u), V(valid_stride), RD(slot_tab, STRIDED(nslots, slot_tab_stride, 2)), V(slot_tab_stride), V(nslots),
      RD(buf_tab, 8u * nbufs), V(nbufs), RD(rows_dev, 0), V(node_stride), T(max_rows), WR(node_words, (size_t)4u * nbufs * node_stride), WR(tracks, (size_t)16u * tracks_cap),
      V(tracks_cap), WR(stats, 16u), WR(scratch, 4u * scratch_u32), V(scratch_u32), FITS(records, 16u * (uint64_t)max_n, rec_slot_stride),
      FITS(masks, masks ? max_n : 0u, mask_slot_stride);
  if (sim_roles && (uint64_t)nbufs * max_rows / 2u > tracks_cap)
    slot_fits("tracks: nbufs * max_rows / 2 records against tracks_cap", (uint64_t)nbufs * max_rows / 2u, tracks_cap, 2);
  END;
}
