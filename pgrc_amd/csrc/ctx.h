// ctx.h -- shared declarations of libpgrc_match.so (host side of the HIP path).
//
// Data layout in HBM:
//   pg2[strand]   u32[ceil(G/16)+PG_PAD]   2-bit text, symbol i at bits 2*(i%16) of word i/16
//   reads2        u32[NW][stride]          word-major ("transposed") reads: thread i of a wave
//                                          reads word w of read i at reads2[w*stride+i] => every
//                                          wave-level load is one coalesced 256-B line
//   head          2 x u64[hash_size]       the bucket's two smallest entries (pos << 22 | 22-bit fingerprint); for
//                                          buckets with >= 3 entries w0 carries a flag, w1 the count and the index
//                                          of entry 1 in ent[]: one 16-B gather per probe (copmem.hip)
//   ent           u64[sampled positions]   all entries sorted by (bucket, position): the build's radix-sort output
//                                          (head and ent of one strand: a PgrcIndexSet; a context has two, and the runs that
//                                          keep both strands' indexes put both sets' heads into one pair table, headfmt.h)
//   pos/rc/mism   u64[n] / u8[n] / u8[n]   per-read results (ReadsMatchers.h:32-35,115)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pgrc_match.h"

#define PGRC_PG_PAD_WORDS 32u   // zero words after the text so NW+1-word windows never fault
#define PGRC_MAX_NW 16          // ceil(255/16)
#define PGRC_BUCKET_CAP 13u     // HASH_COLLISIONS_PER_POSITION_LIMIT + 1 (CopMEMMatcher.h:11)
#define PGRC_TRUNC_BUCKET 4u    // UNLIMITED_NUMBER_OF_HASH_COLLISIONS_PER_POSITION (CopMEMMatcher.h:13)

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};
// A struct names its device buffers once, in a function that returns this list: whoever frees them, or needs all of them, walks it
typedef std::vector<DevBuf *> DevBufList;

// What every context is on the device side: its device, the stream its work is ordered on and the text of its last
// error.  The shared services (the allocators below, pack.hip, radix.hip, pgrc_ps_scan_u32) need nothing else.
struct PgrcDev {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
};

// HIP failure -> ABI error code: out of memory is PGRC_E_ALLOC, a missing / invalid device PGRC_E_NO_DEVICE, anything
// else (launch failure, invalid value, ...) PGRC_E_DEVICE
static inline int pgrc_hip_code(hipError_t e) {
    if (e == hipErrorOutOfMemory) return PGRC_E_ALLOC;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return PGRC_E_NO_DEVICE;
    return PGRC_E_DEVICE;
}

// A stream beside the context's own, with the NEV events (one or two) that order it against the others: made on first use, all
// of it or nothing, and given back with the context.  Work is queued on it by passing `stream` to whoever launches: nothing
// ever stands in for a context's own stream.
template <int NEV = 2>
struct PgrcAuxStream {
    hipStream_t stream = nullptr;
    hipEvent_t ev[NEV]{};
    int ensure(PgrcDev *c, const char *what) {      // on failure: "<what>: <HIP's text>" in c->err, and nothing made
        if (stream) return PGRC_OK;
        hipError_t he = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        for (int k = 0; k < NEV && he == hipSuccess; k++) he = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
        if (he == hipSuccess) return PGRC_OK;
        release();
        c->err = std::string(what) + ": " + hipGetErrorString(he);
        return pgrc_hip_code(he);
    }
    void release() {
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
        for (hipEvent_t &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
};

struct pgrc_multi;   // multi.hip

// One strand's copMEM index as the build leaves it.  A context has two of them (pgrc_match_ctx::idx): the plain passes
// rebuild one per pass, the screened schedule and the dual kernel keep the forward index in one and the RC index in the other.
struct PgrcIndexSet {
    DevBuf head;                        // ulonglong2[hash_size] bucket heads: this set's own table of 16-byte heads
    DevBuf skey[2], sval[2], sorttmp;   // (bucket, entry) records: the build's ping-pong buffers and its scratch (grow-only)
    ulonglong2 *head_ptr = nullptr;     // head h at head_ptr[head_slot(h, head_sh)] (headfmt.h): into `head` (head_sh = 0) or
    uint32_t head_sh = 0;               // into the context's pair table, which both sets share
    const uint64_t *ent = nullptr;      // the sorted entries (one of sval[]), ent[] of the match kernels; set when the build is queued whole
    int strand = -1;                    // which strand's text the set describes; -1: nothing
};

// The reads a match launch works on: [lo, lo + n) of the set (clipped to it); skip_n: the reads with N are left to a later
// pass.  The default is everything; a streamed run (stream.hip) launches block by block.
struct PgrcReadRange {
    uint64_t lo = 0, n = ~0ull;
    bool skip_n = false;
};

// Run-time options of a context.  The environment is read ONCE, when the context is created (pgrc_options_from_env,
// api.hip) -- never at a launch -- so a production matcher does not change schedule because somebody's environment
// changes under it; pgrc_match_reload_options(ctx) reads it again (tests and A/B tools that toggle a knob of a live
// context).  include/pgrc_match.h documents every variable.  None of them changes a result.
struct PgrcOptions {
    int dual = -1;                  // PGRC_DUAL        -1 the library's choice, 0 never, 1 whenever the dual kernel applies
    int screen = -1;                // PGRC_SCREEN      -1 not asked for, 0 never, 1 whenever the screened schedule applies
    bool early_stop = true;         // PGRC_EARLY_STOP=0: every read probes all its seeds, as the reference does
    bool round_skip = true;         // PGRC_ROUND_SKIP=0: the dual kernel probes every seed up to the early stop (no round skip)
    bool dual_pack = true;          // PGRC_DUAL_PACK=0: the dual kernel stores a finished read's pos, rc and mism apart (no packed word, no unpack pass)
    bool builds_in_turn = false;    // PGRC_BUILD_STREAMS=1: the two index builds of a two-strand run on one stream
    uint32_t head_pair = 4;         // PGRC_HEAD_PAIR   0: a head table per strand; 1..4: pair table with groups of 1, 2, 4, 8 buckets
    int index_front = 0;            // PGRC_INDEX_SORT  0 "sweep" (idxsweep.hip), 1 "own" (idxsort.hip's stable scatter passes)
    bool index_finish_general = false;   // PGRC_INDEX_FINISH=general: the general finish kernel for every partition
    int index_cfg = -1;             // PGRC_INDEX_CFG=0  the passes of the index build without the XCD-aware tile order (A/B runs)
    bool match_stage = true;        // PGRC_MATCH_STAGE=0: refilling lanes load their own read (k_copmem_match_sm)
    bool nread_inline = true;       // PGRC_NREAD_INLINE=0: every read with an N takes the byte path
    bool force_pos64 = false;       // PGRC_FORCE_POS64=1: the 64-bit-position kernels on a small text (tests)
    bool test_no_second_index = false;   // PGRC_TEST_NO_SECOND_INDEX: the second index set "does not fit" (tests)
    bool stream_timing = false;     // PGRC_STREAM_TIMING: milestones of a streamed run on stderr
    bool host_pack = true;          // PGRC_HOST_PACK=0: an ASCII text goes up as bytes and a kernel packs it (rounds 1-4); default: host threads pack it into pinned buffers
    uint32_t host_threads = 0;      // PGRC_HOST_THREADS: host threads that pack the text (0 = up to 8)
    uint64_t upload_chunk_mb = 0;   // PGRC_UPLOAD_CHUNK_MB: staging chunk of append_reads_* (0 = 256, or 1024 for a streamed run)
    int seed_filter = -1;           // PGRC_SEED_FILTER  modes d/i/e: -1 where it pays, 0 never, 1 always
    uint32_t test_segment_top_bits = 0;   // PGRC_TEST_SEGMENT_TOP_BITS: the segment sort's short way over this many top bits (tests: 8 makes it fail and the long way run)
    uint64_t test_pack_chunk = 0;   // PGRC_TEST_PACK_CHUNK: symbols per chunk of the host packer (tests: a small text runs many chunks; 0 = 32 Mi)
    int seed_heavy_form = 1;        // PGRC_SEED_HEAVY_FORM=window|grouped: heavy windows a wave each / grouped by their key (default)
    int seed_sort = -1;             // PGRC_SEED_SORT=full|segments: how modes d/i/e sort their (key, entry) pairs (-1: by the batch's size)
    uint32_t seed_heavy = 0;        // PGRC_SEED_HEAVY   modes d/i/e: entries of a window above which the persistent grid expands it (0 = default)
    uint64_t seed_read_batch = 0;   // PGRC_SEED_READ_BATCH / PGRC_SEED_SEGMENT: reads per batch / window starts per launch (tests; 0 = default)
    uint64_t seed_segment = 0;
    uint64_t mem_event_cap = 0;     // PGRC_MEM_EVENT_CAP: first guess of the Pg-vs-Pg matcher's event buffer (tests; 0 = default)
    int allgather = 0;              // PGRC_ALLGATHER    multi-device contexts: 0 by device list, 1 "rccl", 2 "copy" (tests)
};
PgrcOptions pgrc_options_from_env();
bool pgrc_pack_ascii_host(const uint8_t *src, uint64_t count, uint32_t *dst, uint32_t threads);   // api.hip: ASCII ACGT -> 2-bit words, false = a symbol outside ACGT

// The chunked upload of a read set (pgrc_match_begin_reads / _append_ / _end_, api.hip): what one begin .. end sequence
// collects, and the staging it reuses from one sequence to the next.
struct PgrcUpload {
    bool open = false;                          // between begin_reads and end_reads
    uint64_t next = 0;                          // rows appended so far
    uint64_t chunk = 0;                         // staging chunks so far: chunk k goes through stage[k & 1] and, in a streamed run, stream[k & 1]
    std::vector<uint32_t> nidx;                 // reads with N seen so far (ascending)
    uint64_t nmany = 0;                         // ... of them with more than 4 N's
    std::vector<DevBuf> nchunks;                // their ASCII rows, one device buffer per appended block that had some
    std::vector<uint64_t> nchunk_rows;
    DevBuf flag, lidx;                          // bad-symbol flag, positions of a block's N rows (kept: freeing a small buffer goes to
                                                // hipFree, which waits for the whole device -- i.e. for the matching of a streamed run)
    DevBuf stage[2];                            // staging areas (grow-only: no allocation per call), used in turn
    // stream[0]: begin_reads clears the N flags beside index builds queued on the main stream.  A streamed run uploads and unpacks
    // beside the matching, on both in turn: the copy of chunk k+1 must not queue behind the unpacking of chunk k, which waits for a
    // free CU while the persistent match kernel of chunk k-1 runs.  ev[0] of each: "this chunk is unpacked" (stream.hip)
    PgrcAuxStream<1> stream[2];
    DevBufList bufs() { return {&flag, &lidx, &stage[0], &stage[1]}; }
    void reset();                               // a new sequence: nothing appended, no reads with N (api.hip)
};

// A streamed run (stream.hip, the only file that touches the members): blocks of reads matched as they arrive, their results
// downloaded by a worker thread.  Others ask pgrc_stream_active and call the functions declared under "stream.hip" below.
struct PgrcStreamRun {
    struct StreamBlock { uint64_t lo, cnt; hipEvent_t done; };
    bool on = false, dual = false;
    uint64_t *pos = nullptr;            // the caller's result arrays: a block's results are copied there as soon as they exist
    uint8_t *rc = nullptr, *mism = nullptr;
    std::vector<DevBuf> keep;           // small device buffers to give back at the run's end (pgrc_stream_release_bufs)
    hipEvent_t ready = nullptr;         // indexes built and per-read state initialised (what the N passes wait for)
    std::thread worker;                 // downloads finished blocks while the caller uploads the next ones
    std::mutex mu;
    std::condition_variable cv;
    std::deque<StreamBlock> q;
    bool quit = false;
    int err = 0;
    std::vector<std::pair<uint64_t, uint64_t>> nblocks;   // blocks holding reads with N: downloaded again at the end
    double t0 = 0;                      // host clock at stream_begin (ms_total, PGRC_STREAM_TIMING)
    hipEvent_t tbase = nullptr;         // PGRC_STREAM_TIMING: device times of the blocks' match launches
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tev;
};

// The read-side seed index of modes d / i / e (seedidx.hip)
struct PgrcSeedBufs {
    DevBuf keys, vals, tab, hits, tmp, sort, seg, hv, hvu;
    DevBuf filter;          // one bit per slice of the key space
    DevBuf nmask;           // N masks of the reads with N
    DevBuf best, rows;      // the atomic-minimum reduction: one key per read, the batch's reads row by row (seedidx.hip 3c)
    DevBufList bufs() { return {&keys, &filter, &vals, &tab, &hits, &tmp, &sort, &seg, &hv, &hvu, &nmask, &best, &rows}; }
};

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                 \
            return pgrc_hip_code(e__);                                                       \
        }                                                                                    \
    } while (0)

static float dec_elapsed(hipEvent_t a, hipEvent_t b) {       // 0 if either event was never recorded
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return ms;
}
static inline float dec_ms_since(std::chrono::steady_clock::time_point t0) {   // host time since t0
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The timing events of a call's phases: made on first use, recorded on a stream, read in pairs, given back with the context
template <int N>
struct PhaseEvents {
    hipEvent_t ev[N]{};
    int ensure(PgrcDev *c) {
        for (hipEvent_t &ev : this->ev)
            if (!ev) HIP_TRY(c, hipEventCreate(&ev));
        return PGRC_OK;
    }
    hipError_t record(int k, hipStream_t stream) { return hipEventRecord(ev[k], stream); }
    float ms(int a, int b) const { return dec_elapsed(ev[a], ev[b]); }
    void release() {
        for (hipEvent_t &ev : this->ev) {
            if (ev) (void)hipEventDestroy(ev);
            ev = nullptr;
        }
    }
};

// The text of a context: both strands as 2-bit words (the layout above)
struct PgrcText {
    uint64_t G = 0;
    uint64_t pg_words = 0;  // ceil(G / 16)
    DevBuf pg2[2];          // [0] forward, [1] reverse complement
    bool have_pg = false, have_rc = false;
    DevBufList bufs() { return {&pg2[0], &pg2[1]}; }
};

// The read set of a context
struct PgrcReadSet {
    uint64_t n = 0, stride = 0;
    uint32_t nw = 0;
    DevBuf reads_own;       // owned copy (set_reads_ascii / _packed)
    const uint32_t *reads2 = nullptr; // active pointer (owned or borrowed)
    bool have_reads = false;
    // reads with 'N': byte path
    uint64_t n_nreads = 0;
    DevBuf nread_idx;       // u32[n_nreads] read index
    DevBuf nread_ascii;     // u8[n_nreads][read_len]
    DevBuf nread_flag;      // u8[n] 0 = no N; 1 = N's, the byte path (k_copmem_match_n); 3 = at most 4 N's: their positions are in
                            // nread_npos and the dual kernel takes the read itself (the other schedules treat 3 like 1)
    DevBuf nread_npos;      // u32[n] four position bytes (0xFF = none) of the reads flagged 3 (pack.hip, k_npos_rows)
    uint64_t n_many = 0;    // reads flagged 1: more N's than the dual kernel takes
    std::vector<uint32_t> h_nidx; // host copy of nread_idx (ascending): modes d/i/e cut it per batch of reads
    DevBufList bufs() { return {&reads_own, &nread_idx, &nread_ascii, &nread_flag, &nread_npos}; }
};

// What a run leaves: the per-read results, their histogram, the device counter block (PgrcDevCounters, matchdev.h)
struct PgrcResults {
    DevBuf d_pos, d_rc, d_mism, d_hist, d_counters;
    DevBuf d_scr_pos, d_scr_flag;       // per read the flag / position the screen found (screened schedule and dual kernel)
    bool have_results = false;
    uint64_t hist[256]{};
    uint64_t matched = 0;
    DevBufList bufs() { return {&d_pos, &d_rc, &d_mism, &d_hist, &d_counters, &d_scr_pos, &d_scr_flag}; }
};

// The boundaries between the timed phases of a run (pgrc_match_run / _run_pass, api.hip), each an event on the main stream.
// Which of them a run marks depends on its schedule; the ms_* fields of pgrc_match_counters are spans between them
// (run_phase_times, api.hip).
enum PgrcBoundary {
    TM_RUN_START,
    TM_RC_TEXT,             // both indexes in one go: the RC text is made, the builds begin (prepared indexes: the wait for them)
    TM_FW_INDEX,            // ... builds in turn only: the forward index is built
    TM_BOTH_INDEXES,        // ... both are (builds on two streams: the main stream has waited for the second)
    TM_SCHEDULE,            // the screen, or the dual kernel, is through the reads
    TM_PASS_BEGIN,          // + 3 * strand: a pass of its own begins (the RC pass: its RC text is made),
    TM_PASS_INDEX,          //               has its index,
    TM_PASS_MATCHED,        //               is through the reads
    TM_RUN_END = TM_PASS_BEGIN + 6,
    TM_COUNT
};
// The timer of a run: made by pgrc_match_set_profiling, and off (nothing recorded) outside a run with profiling on
struct PgrcRunTimer {
    PhaseEvents<TM_COUNT> ev;
    uint32_t marked = 0;    // the boundaries this run marked: an event of an earlier run with another schedule is not read
    bool on = false;
    int ensure(PgrcDev *c) { return ev.ensure(c); }
    void begin(bool profiling) { on = profiling && ev.ev[0]; marked = 0; }
    void mark(int b, hipStream_t stream) {
        if (!on) return;
        (void)ev.record(b, stream);
        marked |= 1u << b;
    }
    bool has(int b) const { return marked >> b & 1u; }
    float ms(int a, int b) const { return has(a) && has(b) ? ev.ms(a, b) : 0.f; }   // 0: not recorded
};

struct pgrc_match_ctx : PgrcDev {
    PgrcOptions opt;                    // read from the environment by pgrc_match_create (see above)

    // several devices behind this object (pgrc_match_create_multi): it is then only the front, the work happens in
    // one child context per device
    pgrc_multi *multi = nullptr;
    void *export_view = nullptr;        // multi-device front: the shards' results gathered on the first device (export.hip)
    pgrc_match_ctx *export_front = nullptr;   // set in that gathered view: the front whose shards hold the reads (mismatch lists per shard)

    pgrc_match_params prm{};
    int num_cus = 256;
    PgrcAuxStream<2> side;              // the kernel for reads with N runs beside the main match kernel: ev[0] "the main stream is
                                        // ready for it", ev[1] "it is done"

    PgrcText txt;           // pseudogenome
    PgrcReadSet rd;         // reads
    PgrcUpload up;          // chunked upload (pgrc_match_begin_reads / _append_ / _end_)

    PgrcResults res;        // per-read results, their histogram, the device counters

    // copMEM index (rebuilt per pass, buffers reused)
    pgrc_copmem_params cp{};
    uint64_t npos = 0;
    // The two index sets (PgrcIndexSet above).  A build writes into idx[build_set]; a launch looks its strand up
    // (pgrc_index_of).  A context that never keeps both strands' indexes only ever owns the buffers of one set; the
    // schedules that do (copmem.hip, "Exact-match screen" and "The dual kernel") turn build_set between their two builds.
    PgrcIndexSet idx[2];
    int build_set = 0;
    // The pair table (round 4, runs that keep both strands' indexes): the forward and the RC head of a bucket number share
    // a line -- the dual kernel's two gathers of a seed are then ONE line request and one translation (copmem.hip, "The
    // dual kernel").  Shared by both sets: a set whose head_sh != 0 has its heads here.
    DevBuf d_headpair;                  // ulonglong2[2 * hash_size]
    uint32_t pair_gm = 3;               // pair table: buckets per group - 1 (a power of two minus one; headfmt.h)
    bool os_lds_allowed = false;        // idxsweep.hip's kernels were granted their dynamic LDS on this context's device
    bool screen_broken = false;         // no room for the second set: the passes run as the reference orders them
    PgrcAuxStream<2> build;             // the RC index is built beside the forward one: ev[0] "the RC text is ready", ev[1] "the
                                        // RC index is built" (pgrc_build_both_indexes, api.hip)

    // pipelined hand-over (stream.hip): both indexes built ahead of the run; blocks of reads matched as they arrive
    bool idx_prepared = false;          // pgrc_match_prepare_index built (or is building) both strands' indexes of the current text
    PgrcStreamRun st;

    PgrcSeedBufs seed;      // modes d / i / e

    // profiling
    bool profiling = false;
    pgrc_match_counters ctr{};
    PgrcRunTimer tm;
};

// Every ABI entry point runs on its context's device and leaves the caller's current device (e.g. torch's) as it
// found it.
struct PgrcDeviceScope {
    int prev = -1;
    bool ok = true;
    explicit PgrcDeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev == dev) prev = -1;                       // nothing to switch, nothing to restore
        else ok = hipSetDevice(dev) == hipSuccess;
    }
    ~PgrcDeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
#define PGRC_ON_DEVICE(ctx)                                                                  \
    PgrcDeviceScope dev_scope__((ctx)->device);                                              \
    if (!dev_scope__.ok) {                                                                   \
        (ctx)->err = "hipSetDevice(" + std::to_string((ctx)->device) + ") failed";           \
        return PGRC_E_NO_DEVICE;                                                             \
    }

// the pooled allocator (api.hip): grow-only, rounded up, and what it gives back goes to the process-wide pool
int pgrc_buf_ensure(PgrcDev *c, DevBuf &b, size_t bytes);
void pgrc_buf_free(DevBuf &b);
void pgrc_buf_free_all(DevBuf *const *bufs, size_t count);   // one wait for the device for the whole batch
// the unpooled one: grow-only, exactly `bytes` (64 at least) from hipMalloc, given back with dec_free
int pgrc_buf_unpooled(PgrcDev *c, DevBuf &b, size_t bytes);
bool pgrc_host_pinned(const void *p);   // a host pointer that HIP knows as page-locked: copies to and from it need no staging

static void dec_free(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

// the unpooled buffers of a context (its list, above), given back by its destroy function
static void dec_free_all(const DevBufList &bufs) {
    for (DevBuf *b : bufs) dec_free(*b);
}

// pgrc_buf_unpooled for every {buffer, bytes} in turn; the first error ends it
static int pgrc_bufs_unpooled(PgrcDev *c, std::initializer_list<std::pair<DevBuf *, size_t>> want) {
    for (const auto &w : want)
        if (int e = pgrc_buf_unpooled(c, *w.first, w.second)) return e;
    return PGRC_OK;
}

// api.hip: (re)allocates and clears both strands' text buffers for a text of G symbols
extern "C" int pgrc_pg_alloc(pgrc_match_ctx *c, uint64_t G);

// multi.hip: the front context's side of every entry point
int pgrc_multi_set_pg_ascii(pgrc_match_ctx *f, const char *pg, uint64_t G);
int pgrc_multi_set_pg_packed_device(pgrc_match_ctx *f, const void *d_words, uint64_t G);
int pgrc_multi_pack_pg_slice(pgrc_match_ctx *f, const char *pg, uint64_t count, void *d_words_out);
int pgrc_multi_begin_reads(pgrc_match_ctx *f, uint64_t n);
int pgrc_multi_append_reads(pgrc_match_ctx *f, const void *rows, uint64_t count, int32_t symbols /* 0 = ASCII */);
int pgrc_multi_end_reads(pgrc_match_ctx *f);
int pgrc_multi_set_reads_device(pgrc_match_ctx *f, const void *d_words, uint64_t n, uint64_t stride);
int pgrc_multi_init_results(pgrc_match_ctx *f);
int pgrc_multi_set_results(pgrc_match_ctx *f, const uint64_t *pos, const uint8_t *rc, const uint8_t *mism);
int pgrc_multi_run(pgrc_match_ctx *f, int first, int last);
int pgrc_multi_get_results(pgrc_match_ctx *f, uint64_t *pos, uint8_t *rc, uint8_t *mism, uint64_t hist[256], uint64_t *matched);
int pgrc_multi_extract_mismatches(pgrc_match_ctx *f, const uint8_t *reversed_flags, uint64_t *cum, uint8_t *codes,
                                  uint16_t *offsets);
int pgrc_multi_export_index(pgrc_match_ctx *f, int strand, uint32_t *cumm, uint32_t *positions, uint64_t *count);
int pgrc_multi_export_pg(pgrc_match_ctx *f, int strand, uint32_t *words);
int pgrc_multi_set_profiling(pgrc_match_ctx *f, int enabled);
int pgrc_multi_get_counters(pgrc_match_ctx *f, pgrc_match_counters *out);
void pgrc_multi_destroy(pgrc_match_ctx *f);
struct PgrcShardView { pgrc_match_ctx *ctx; uint64_t lo, hi; };     // one shard of a multi-device context: reads [lo, hi)
std::vector<PgrcShardView> pgrc_multi_shards(pgrc_match_ctx *f);
void pgrc_export_drop_view(pgrc_match_ctx *front);   // export.hip: forget the gathered view (text, reads or results change)

// pack.hip: each queues its kernel on `stream` (c: the error text)
int pgrc_launch_pack_ascii(PgrcDev *c, hipStream_t stream, const uint8_t *d_ascii, uint64_t count, uint32_t *d_words,
                           uint32_t *d_errflag);
int pgrc_launch_revcomp(PgrcDev *c, hipStream_t stream, const uint32_t *d_fw, uint32_t *d_rc, uint64_t G);
int pgrc_launch_pack_reads_ascii(PgrcDev *c, hipStream_t stream, const uint8_t *d_ascii, uint64_t first, uint64_t count,
                                 uint32_t L, uint32_t *d_words, uint64_t stride, uint8_t *d_nflag,
                                 uint32_t *d_errflag);
int pgrc_launch_repack_reads_ref(PgrcDev *c, hipStream_t stream, const uint8_t *d_packed, uint64_t first, uint64_t count,
                                 uint32_t L, uint32_t *d_words, uint64_t stride);
int pgrc_launch_unpack_reads_acgnt(PgrcDev *c, hipStream_t stream, const uint8_t *d_packed, uint64_t first, uint64_t count,
                                   uint32_t L, uint32_t *d_words, uint64_t stride, uint8_t *d_nflag, uint32_t *d_errflag);
int pgrc_launch_npos_rows(PgrcDev *c, hipStream_t stream, const uint8_t *d_rows, int symbols, uint64_t first, uint64_t count, uint32_t L,
                          uint8_t *d_nflag, uint32_t *d_npos);
int pgrc_launch_nrows_ascii_acgnt(PgrcDev *c, hipStream_t stream, const uint8_t *d_packed, const uint32_t *d_local_idx, uint64_t count,
                                  uint32_t L, uint8_t *d_ascii);

// mempack.hip: an ASCII text in HBM (any byte alignment) -> words_out 2-bit words (zero behind the text), the N map (or null)
// and the flag word (bit 0 a symbol outside ACGNT, bit 1 an N; the caller clears it), forward or reverse-complemented, in
// one launch of at most block_cap blocks (0: the usual 65 536)
int pgrc_launch_mem_pack_device(PgrcDev *c, const uint8_t *d_ascii, uint64_t n, bool reversed, uint32_t *d_words, uint16_t *d_nmap, uint64_t words_out,
                                uint32_t *d_flags, uint32_t block_cap);

// copmem.hip
// Builds go to the build set, launches look a strand up:
static inline PgrcIndexSet &pgrc_build_set(pgrc_match_ctx *c) { return c->idx[c->build_set]; }   // what the next build writes into
PgrcIndexSet *pgrc_index_of(pgrc_match_ctx *c, int strand);   // the finished set of that strand (the build set first), or null
bool pgrc_index_pair_ready(pgrc_match_ctx *c);                 // a set for either strand, their heads in the same kind of table
void pgrc_index_drop(pgrc_match_ctx *c, PgrcIndexSet &ix);     // frees the set's buffers; it describes nothing afterwards
void pgrc_index_retreat(pgrc_match_ctx *c);                    // no room for the second set: see its definition
// into_pair_table: the heads go into the strand's half of the pair table (the builds of a run that keeps both indexes)
// The build path queues on the stream it is given (the context's own, or its build stream for the second of two builds at once)
int pgrc_copmem_build_index(pgrc_match_ctx *c, hipStream_t stream, int strand, bool into_pair_table = false);
// idxsort.hip: the partition build of the same index (hand-written scatter passes, in-LDS finish of a partition)
uint32_t pgrc_ps_partition_bits(uint32_t hbits);
bool pgrc_ps_applicable(const pgrc_match_ctx *c, uint32_t hbits);
int pgrc_ps_scatter_front(pgrc_match_ctx *c, hipStream_t stream, int strand, uint32_t hbits, uint32_t cb);
int pgrc_ps_finish(pgrc_match_ctx *c, hipStream_t stream, const uint32_t *d_keys, const uint64_t *d_vals, uint32_t hbits, uint32_t cb, uint64_t *d_ent);
int pgrc_ps_finish_packed(pgrc_match_ctx *c, hipStream_t stream, const uint64_t *d_recs, const uint32_t *d_pstart, uint32_t *d_slow, uint32_t np, uint32_t cb,
                          uint32_t rec_sh, uint64_t *d_ent);
// the shared scan (scanops.h) in place over u32 counts, exclusive; d_fold: pgrc_ps_scan_blocks(n) words of scratch
uint64_t pgrc_ps_scan_blocks(uint64_t n);
int pgrc_ps_scan_u32(PgrcDev *c, hipStream_t stream, uint32_t *d_io, uint64_t n, uint32_t *d_fold);
// idxsweep.hip: the default front end (one-sweep scatter passes that hash the text themselves, 8-byte records)
bool pgrc_os_applicable(const pgrc_match_ctx *c, uint32_t hbits);
int pgrc_os_build_index(pgrc_match_ctx *c, hipStream_t stream, int strand, uint32_t hbits);
int pgrc_copmem_match_pass(pgrc_match_ctx *c, int strand);
// stream.hip: what the rest of the matcher sees of a streamed run
bool pgrc_stream_active(const pgrc_match_ctx *c);
// a block of reads just arrived on the device (append_reads_*, unpacking queued on up.stream[turn]): match it now if streaming is on
int pgrc_stream_block_arrived(pgrc_match_ctx *c, uint64_t lo, uint64_t cnt, bool may_hold_n, int turn);
void pgrc_stream_abort(pgrc_match_ctx *c);
void pgrc_stream_release(pgrc_match_ctx *c);   // ... and its events given back (pgrc_match_destroy)
// gives small device buffers back and empties the list: at once, or -- they go to hipFree, which waits for the whole device, i.e. for
// the matching -- at the end of the streamed run that is on
void pgrc_stream_release_bufs(pgrc_match_ctx *c, std::vector<DevBuf> &bufs);
// PGRC_STREAM_TIMING: a milestone of the streamed run that is on, on stderr with the host time since stream_begin
void pgrc_stream_mark(pgrc_match_ctx *c, const char *what);
// api.hip
int pgrc_make_rc_text(pgrc_match_ctx *c, hipStream_t stream);   // the RC text from the forward one, queued on `stream` (what every run does)
int pgrc_need_rc_text(pgrc_match_ctx *c);                       // ... on the context's stream, and only if it is missing (the exports)
int pgrc_counters_clear(pgrc_match_ctx *c);                     // a run begins: the device counter block and c->ctr are zero
void pgrc_upload_close(pgrc_match_ctx *c);   // a begin .. end sequence that failed does not stay open: no reads until the next begin_reads
int pgrc_prepare_both_indexes(pgrc_match_ctx *c);
bool pgrc_dual_applies(const pgrc_match_ctx *c);
int pgrc_fetch_schedule_counters(pgrc_match_ctx *c, bool dual);   // the dual kernel's (or the screen's) device counters -> c->ctr
int pgrc_copmem_match_phase(pgrc_match_ctx *c, int strand, int phase, PgrcReadRange range = {});
int pgrc_copmem_match_dual(pgrc_match_ctx *c, PgrcReadRange range = {});
// after: the N kernel's side stream waits for this event instead of the main stream's tail
int pgrc_copmem_match_nreads(pgrc_match_ctx *c, int first, int last, bool only_many, hipEvent_t after = nullptr);
int pgrc_copmem_join_nreads(pgrc_match_ctx *c);
int pgrc_copmem_export_index(pgrc_match_ctx *c, int strand, uint32_t *h_cumm, uint32_t *h_positions, uint64_t *count);

// radix.hip: stable LSD radix sort of 64-bit records by the bit field [bit_lo, bit_hi) (hand-written; d_b / k_b / v_b: scratch of n
// records; `scratch` grows as needed; *sorted: wherever the last pass put them); the pairs form carries a 64-bit value per key
int pgrc_radix_sort_u64(PgrcDev *c, uint64_t *d_a, uint64_t *d_b, uint64_t n, uint32_t bit_lo, uint32_t bit_hi, DevBuf &scratch,
                        uint64_t **sorted);
int pgrc_radix_sort_pairs_u64(PgrcDev *c, uint64_t *k_a, uint64_t *k_b, uint64_t *v_a, uint64_t *v_b, uint64_t n, uint32_t bit_lo, uint32_t bit_hi,
                              DevBuf &scratch, uint64_t **ksorted, uint64_t **vsorted);
#define PGRC_RX_SEGMENT_MAX 8192u      // pairs a segment of pgrc_radix_sort_segments_pairs_u64 may hold (radix.hip RX_TILE)
int pgrc_radix_sort_segments_pairs_u64(PgrcDev *c, uint64_t *keys, uint64_t *vals, const uint32_t *seg, uint32_t nseg, uint32_t bit_lo, uint32_t bit_hi,
                                       uint32_t *ovl, uint32_t cap, uint32_t top_bits);

// seedidx.hip (modes d / i / e)
int pgrc_seedidx_run(pgrc_match_ctx *c, int first_strand, int last_strand);

// results.hip
int pgrc_launch_init_results(pgrc_match_ctx *c);
int pgrc_launch_hist(pgrc_match_ctx *c);
// The dual kernel's packed result word in pos[] (dualkern.h, "The packed result"): position (< 2^40: api.hip alloc_pg) |
// count << 40 | strand << 48 | tag.  Bit 62 set and bit 63 clear: neither a plain position (both clear) nor
// PGRC_NOT_MATCHED_POS (both set).
#define RES_PACK_MISM_SHIFT 40
#define RES_PACK_RC_SHIFT 48
#define RES_PACK_TAG (1ull << 62)
#define RES_PACK_POS_MASK ((1ull << 40) - 1ull)
int pgrc_launch_unpack_results(pgrc_match_ctx *c, uint64_t lo, uint64_t n);   // queued on c->stream: reads lo .. lo + n - 1
int pgrc_extract_mismatches(pgrc_match_ctx *c, const uint8_t *reversed_flags, uint64_t *cum, uint8_t *codes,
                            uint16_t *offsets);
int pgrc_extract_lists_device(pgrc_match_ctx *c, const uint8_t *d_revflags, bool lists, DevBuf &d_cum, DevBuf &d_codes, DevBuf &d_offs,
                              uint64_t *total_out);
