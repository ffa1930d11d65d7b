// msastat_batch.hip -- msa_trim_batch: native worker threads with a context each, and the batch engine (one launch per kernel
// family over whole groups of small alignments).
#include "msastat_ctx.h"

using namespace msai;

// The arguments of ONE call of the batch object: msa_trim_batch (ROWS) or msa_trim_batch_fasta[_emit] (TEXTS).  The entry point
// fills one of these completely, run_call copies it into the batch object for the call's duration and clears it at the end: no
// member of one call kind survives into a call of the other.
struct BatchCall {
    enum Kind { NONE, ROWS, TEXTS } kind = NONE;
    int32_t count = 0;
    int32_t *rc = nullptr;
    // ROWS
    const uint8_t *const *data = nullptr;
    const int32_t *m = nullptr, *n = nullptr;
    const int64_t *ld = nullptr;
    const uint8_t *indet = nullptr;
    const msa_trim_params *params = nullptr;
    uint8_t *const *keep_res = nullptr, *const *keep_seq = nullptr;
    msa_trim_info *info = nullptr;
    // TEXTS (what each of them gave: msa_batch::fasta)
    const uint8_t *const *texts = nullptr;
    const int64_t *lens = nullptr;
    const uint8_t *valid = nullptr;
    const msa_trim_params *params_by_type = nullptr;
    bool want_rows = false;
    int emit_format = -1;  // msa_trim_batch_fasta_emit: the MSA_TEXT_* format the workers compose behind the trim, -1 none
};

// ---- batches of independent alignments ----------------------------------------------------------------------------
// The reference's batch idiom is a thread pool over `trimmer.trim` (README.md:136-152), possible because its `trim`
// releases the interpreter lock for the whole computation (_trimal.pyx:1334-1359).  Here the pool is native: worker
// threads, each with its own context (device buffers, streams), take the alignments of a call largest first; a worker
// uploads its alignment without waiting (the caller's rows outlive the call) and trims it, so that the upload of one
// alignment, the kernels of others and the host selection logic of yet others overlap on one GPU, with nothing of the
// interpreter in between.
struct msa_batch {
    // -- the pool: lives as long as the object
    int device = 0;
    std::vector<msa_ctx *> ctxs;
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    uint64_t generation = 0;
    bool stop = false;
    int running = 0;
    bool in_call = false;
    struct Engine *engine = nullptr;              // the batched-kernel path (below), created on first use
    // the engine's host-side loops (packing rows for the upload, the selection step), shared with the workers that have
    // nothing else to do: engine_parallel_for
    uint64_t sel_generation = 0;
    bool sel_open = false;   // (under `mu`) helpers may still join the job
    int sel_active = 0;      // (under `mu`) helpers inside it
    std::function<void(int32_t, int)> sel_fn;  // (item, thread: a worker's index, or workers.size() for the calling thread)
    int32_t sel_total = 0;
    std::atomic<int32_t> sel_next{0};
    std::vector<int32_t> sel_redo;
    std::vector<uint8_t> sel_finished;  // per alignment of the call: the engine has delivered its result
    bool use_engine = true;                       // MSA_BATCH_ENGINE=0: every alignment through the workers (diagnostics, tests)
    double engine_max_work = 3e8;                 // m * m * n up to which the engine takes an alignment (MSA_BATCH_ENGINE_MAX)
    int engine_min_count = 40;                    // fewer eligible alignments than this go to the workers instead (MSA_BATCH_ENGINE_MIN)
    // -- the call in flight (run_call), and the workers' share of it, largest first
    BatchCall call;
    std::vector<int32_t> order;
    std::atomic<int32_t> next{0};
    // -- what a call leaves behind, valid until the next call of either kind
    std::vector<std::vector<int32_t>> only_gaps;  // per alignment: the rows behind MSA_W_ONLY_GAPS_SEQUENCES
    struct FastaResult {
        int parse_rc = MSA_OK;
        msa_text_info info{};
        msa_trim_info tinfo{};
        msa_err_detail detail{};
        std::vector<uint8_t> keep_res, keep_seq, rows;
        std::vector<int64_t> name_off;
        std::vector<int32_t> name_len;
        std::unique_ptr<uint8_t[]> text;  // the composed text (not value-initialised: every byte comes from the download)
        int64_t text_len = -1;            // -1: none
        uint32_t text_flags = 0;          // MSA_TEXT_F_*
    };
    std::vector<FastaResult> fasta;  // per text of the last TEXTS call (none after a ROWS call)
    std::vector<int32_t> routes;     // per alignment of the last ROWS call: MSA_ROUTE_* (msa_batch_debug_routes; none after a TEXTS call)
};

// ---- the batch engine: one launch per kernel family for a whole group of alignments -------------------------------------
// The workers above give every alignment its own ~14 launches, and with four of them in flight the device runs kernels of
// different alignments against each other (profiles/r03_c5_timeline.txt: the kernel durations add up to 3.4 x the window, the
// small layout kernels stretch 4 x).  The engine takes the alignments whose trim is the similarity pipeline of
// sim_pipeline_begin (strict, strictplus, automated1, a manual similarity threshold; no windows; fewer than ~4100 sequences,
// where the pair pass has one regime) in groups: ONE device arena per group laid out alignment after alignment, ONE table of
// descriptors, ONE launch per kernel family with blockIdx -> (alignment, block) through prefix sums, the similarity grid over
// every column of every alignment (each alignment's columns by weight: a counting sort per alignment on the device, behind the
// gap counts), ONE copy of every result vector back, and nothing in between that needs the host.  Two
// groups are in flight: the host takes the selection decisions of group g (trim_impl on a host-only view per alignment)
// while the device works on group g + 1.  Alignments the engine does not take, and the rare alignment whose selection needs
// another pass over the rows, go through the workers / an ordinary context as before.
struct Engine {
    struct Item {
        int32_t k;            // index in the call
        EngineKind kind;      // what its trim needs of the device: decided once per call (engine_takes)
        size_t res_word;      // offset (words) of its block in the result region: flags[16] gaps[npad] indets[npad] rowtot[mpad] mdk[n] q[n]
        int npad, mpad;
        size_t extra_word;    // ... and of what its kind adds behind them (ENGINE_OVERLAP, _REPRESENTATIVE, _DIGESTS)
    };
    struct Lane {
        // two queues per group: uploads and the short VALU-bound kernels (counts, planes, pair pass, lists) at HIGH priority,
        // the similarity kernel behind them at normal priority -- the next group's preparation then gets its workgroups
        // dispatched while this group's similarity grid (tens of thousands of waves, bound by the vector-memory pipeline)
        // is still draining; with one priority the queues take turns and nothing overlaps
        hipStream_t pre = nullptr, stream = nullptr;
        hipEvent_t prepared = nullptr, done = nullptr;
        DevBuf<uint8_t> arena, meta;
        PinBuf<uint8_t> h_meta, h_res, h_stage;
        uint64_t sig = 0;
        std::vector<Item> items;
        bool busy = false;
    };
    static constexpr int MAX_LANES = 4;
    Lane lanes[MAX_LANES];
    int nlanes = 2;             // groups in flight
    bool trace = false;         // MSA_TRACE=1: host-side timing of every group on stderr
    long fetch_max_bytes = 1 << 20;  // page-locked alignments up to this size are fetched by a kernel instead of a copy each
    int cols_max_m = 128;       // groups whose alignments have at most this many sequences: a lane per column (MSA_BATCH_COLS_MAX <= 128)
    msa_ctx *tables = nullptr;  // owns the similarity tables (and trims the alignments that fall back)
    std::vector<msa_ctx *> views;  // the host-only views handed to trim_impl: one per worker, the last one the calling thread's
};

namespace msai {

inline size_t align_up(size_t x, size_t q) { return (x + q - 1) / q * q; }

// what a trim needs of the device (EngineKind, msastat_ctx.h)
EngineKind engine_needs(const msa_trim_params *p) {
    const int method = p->method;
    // the trimmers that remove sequences (round 6): their statistics come back with the group's one copy as well, and the
    // selection runs on the host-only view -- OverlapTrimmer (the overlap counts of every sequence), RepresentativeTrimmer
    // (the identities: clustered on the host, threshold mode and clusters=K alike), noduplicateseqs (row digests)
    if (method == MSA_METHOD_NODUPLICATESEQS) return ENGINE_DIGESTS;
    if (p->clusters != -1 || p->max_identity != -1) return ENGINE_REPRESENTATIVE;
    if (p->residue_overlap != -1 && p->sequence_overlap != -1) return ENGINE_OVERLAP;
    if (method == MSA_METHOD_STRICT || method == MSA_METHOD_STRICTPLUS || method == MSA_METHOD_AUTOMATED1 ||
        (method == MSA_METHOD_NONE && p->similarity_threshold != -1))
        return ENGINE_SIMILARITY;
    if (method == MSA_METHOD_GAPPYOUT || method == MSA_METHOD_NOGAPS || method == MSA_METHOD_NOALLGAPS ||
        (method == MSA_METHOD_NONE && (p->gap_threshold != -1 || p->gap_absolute_threshold != -1)))
        return ENGINE_GAPS;
    return ENGINE_NONE;
}

// Does the engine take alignment k, and as what?  ENGINE_NONE: no.  (the similarity pipeline's conditions, one pair-pass regime,
// 32-bit list offsets, rows the copy engine takes in one piece or that are small enough to pack on the way)
EngineKind engine_takes(const msa_batch *b, int32_t k, const msa_trim_params *ref) {
    const BatchCall &c = b->call;
    const msa_trim_params *p = c.params + k;
    const int m = c.m[k], n = c.n[k];
    if (m < 2 || n < 1 || m > 32768 || !c.data[k] || c.ld[k] < n) return ENGINE_NONE;
    const EngineKind needs = engine_needs(p);
    if (needs == ENGINE_NONE) return ENGINE_NONE;
    int gap_hw = p->gap_window, sim_hw = p->similarity_window;
    if (p->window != -1) gap_hw = sim_hw = p->window;
    // (a gap window is host work on the counts -- unless the similarity pipeline follows: its ">= 80 % gaps" cut reads the windowed
    // counts on the device)
    if (gap_hw > 0 && needs == ENGINE_SIMILARITY) return ENGINE_NONE;
    if (gap_hw > n / 4) return ENGINE_NONE;  // (an error return: the ordinary path reports it)
    if (needs == ENGINE_GAPS || needs == ENGINE_OVERLAP || needs == ENGINE_DIGESTS)
        return (double)m * n <= 4e6 ? needs : ENGINE_NONE;  // (one pass over the rows: small alignments, where launches are the cost)
    if (needs == ENGINE_REPRESENTATIVE) {  // the pair pass, and m x m identities in the group's copy back
        const int m_pad4 = round_up(m, 128);
        return m <= 1024 && msak::pair_pipe_regime(m, m_pad4) && (double)m * m * n <= b->engine_max_work ? needs : ENGINE_NONE;
    }
    if (sim_hw > n / 4) return ENGINE_NONE;
    if (!p->vhash || !p->dist || p->npos < 1 || p->npos > 28) return ENGINE_NONE;
    // one set of tables per call: the first taken alignment's
    if (ref && (ref->npos != p->npos || c.indet[k] != c.indet[ref - c.params] ||
                (ref->vhash != p->vhash && std::memcmp(ref->vhash, p->vhash, 26 * sizeof(int32_t)) != 0) ||
                (ref->dist != p->dist && std::memcmp(ref->dist, p->dist, sizeof(float) * p->npos * p->npos) != 0)))
        return ENGINE_NONE;
    const int m_pad = round_up(m, 128);
    if (!msak::pair_pipe_regime(m, m_pad)) return ENGINE_NONE;
    // Where the batched kernels pay: alignments that do not fill the chip by themselves.  From ~600 x 2500 on a context per
    // alignment (four workers) is as fast or faster -- the similarity kernel bounds both (64 x 1000 x 4000: 23.8 ms of it in
    // either scheme), and four alignments in flight overlap the VALU-bound pair pass of one with the similarity kernel of
    // another, which one launch per family cannot (measured: 26.8 ms against 25.4; 96 x 700 x 3000: 19.7 against 17.5; 1024 x 100 x 1000:
    // 10.2 against 30 through trim_batch).  Since a worker's trim of a small alignment is the compact pipeline the line lies lower:
    // 128 x 500 x 2000 12.8 against 11.7 for the workers, 256 x 300 x 1200 11.0 against 15.2 for the engine.
    // MSA_BATCH_ENGINE_MAX: the m * m * n up to which the engine takes an alignment.
    if ((double)m * m * n > b->engine_max_work) return ENGINE_NONE;
    if ((double)m * m * 12 + (double)msak::bx_cols_pad(n) * msak::bx_ldk(m) * 7 > 6e9) return ENGINE_NONE;  // (a few GB per alignment: one at a time)
    return needs;
}

int engine_parallel_for(msa_batch *b, int32_t total, std::function<void(int32_t, int)> fn);

// fn() with its exceptions as return codes: none may leave a worker thread (std::terminate would take the caller's process
// with it) or the C ABI
template <class F>
static int no_throw(F fn) {
    try {
        return fn();
    } catch (const std::bad_alloc &) {
        return MSA_E_NOMEM;
    } catch (...) {
        return MSA_E_INVALID;
    }
}

// one alignment of a ROWS call on context ctx (a worker's, or the engine's own for a second pass): upload without waiting, trim
static int rows_item(msa_batch *b, msa_ctx *ctx, int32_t k) {
    const BatchCall &c = b->call;
    msa_trim_info local;
    msa_trim_info *info = c.info ? c.info + k : &local;
    ctx->only_gaps_rows.clear();
    int rc = msa_upload_packed_async(ctx, c.data[k], c.m[k], c.n[k], c.ld[k], c.indet[k]);
    if (rc == MSA_OK) {
        rc = msa_trim(ctx, c.params + k, c.keep_res[k], c.keep_seq[k], info);
    } else {
        std::memset(info, 0, sizeof(*info));
        (void)hipStreamSynchronize(ctx->stream);  // (nothing of a failed upload may stay in flight over the caller's rows)
    }
    b->only_gaps[k] = ctx->only_gaps_rows;
    return rc;
}

struct EngineLayout {  // byte offsets of one alignment's arrays in the arena (0: its kind has no such array)
    size_t raw, planes, ident, w, wlow, wbar, row_avg, row_max, codeT, codeR, off, trow, nvalid, simnum, simden, simstate, cols;
};

// What engine_layout decides for one group: where everything lies in the arena, which kernels run, the signature of both.
struct EngineGroup {
    std::vector<EngineLayout> lay;
    size_t res_words = 0, raw_base = 0, raw_bytes = 0, arena_bytes = 0;
    int max_m = 0, any_sim = -1;  // (over the alignments that run the similarity pipeline)
    bool multi = false, cols_mode = false, sort_cols = false;
    uint64_t sig = 1469598103934665603ull;
    void mix(uint64_t v) { sig = (sig ^ v) * 1099511628211ull; }
    // how each alignment's rows reach the arena (engine_row_routes): packed into the staging buffer, fetched by a kernel
    // (page-locked rows as the device sees them: read by fetch_rows_batch_kernel), or neither -- a copy of its own
    std::vector<uint8_t> packed;
    std::vector<const uint8_t *> fetch;
    bool any_packed = false;
};

// the kernel families of a group: one prefix-sum array of blocks each (F_ENCODE / F_COLS: by mode)
enum { F_FETCH, F_GAPS, F_ROWTOT, F_PLANES, F_PAIRS, F_WMEANS, F_IDROWS, F_ENCODE, F_COMPACT, F_FINISH, F_COLS, F_OVERLAP, F_DIGEST, F_COUNT };

// the metadata block of a group of K: [BAlign K][LgAlign K][prefix arrays: F_COUNT x (K + 1)], on the host and on the device
struct EngineMeta {
    msak::BAlign *bt;
    msak::LgAlign *lt;
    int32_t *pf;
};
static size_t engine_meta_bytes(int K) {
    return align_up((size_t)K * sizeof(msak::BAlign), 256) + align_up((size_t)K * sizeof(msak::LgAlign), 256) +
           align_up((size_t)F_COUNT * (K + 1) * sizeof(int32_t), 256);
}
static EngineMeta engine_meta(uint8_t *base, int K) {
    uint8_t *lt = base + align_up((size_t)K * sizeof(msak::BAlign), 256);
    return {reinterpret_cast<msak::BAlign *>(base), reinterpret_cast<msak::LgAlign *>(lt),
            reinterpret_cast<int32_t *>(lt + align_up((size_t)K * sizeof(msak::LgAlign), 256))};
}

// The arena layout of a group: the result region first (one memset, one copy), then the rows of every alignment side by side,
// then the derived arrays.  Fills the items' places in the result region.
static EngineGroup engine_layout(const BatchCall &c, const Engine *e, std::vector<Engine::Item> &items) {
    const int K = (int)items.size();
    EngineGroup g;
    g.lay.assign(K, EngineLayout{});
    for (int i = 0; i < K; ++i) {
        Engine::Item &it = items[i];
        const int m = c.m[it.k], n = c.n[it.k];
        it.npad = round_up(n + 64, 64);
        it.mpad = round_up(m + 64, 64);
        it.res_word = g.res_words;
        g.res_words += 16 + (size_t)2 * it.npad + it.mpad + (size_t)2 * it.npad;
        if (it.kind == ENGINE_SIMILARITY) g.max_m = std::max(g.max_m, m), g.any_sim = i;
        // what the kind brings back beside the common vectors: overlap counts [mpad]; identities [m][ldw]; lengths [mpad] + hashes
        it.extra_word = g.res_words;
        g.res_words += it.kind == ENGINE_OVERLAP          ? (size_t)it.mpad
                       : it.kind == ENGINE_REPRESENTATIVE ? (size_t)m * round_up(m, 64)
                       : it.kind == ENGINE_DIGESTS        ? (size_t)5 * it.mpad
                                                          : 0;
        g.mix(((uint64_t)(uint32_t)m << 32) | (uint32_t)n);
        g.mix(c.params[it.k].method == MSA_METHOD_AUTOMATED1);
        g.mix(it.kind);
    }
    g.multi = msak::lg_rounds_per_launch(g.max_m) > 0;  // (the similarity kernel in several launches: per-column state)
    // groups of small alignments: the similarity statistic with a lane per column (similarity_cols_batch_kernel) -- no
    // column-major codes, no lists
    g.cols_mode = g.max_m <= e->cols_max_m;
    g.mix(g.cols_mode);
    // the wave-per-column kernel's columns dealt by weight, alignment by alignment (a counting sort per alignment on the device,
    // behind the gap counts: workgroups of four columns of like weight, the heaviest first -- over the columns as they lie a
    // workgroup's slots are held until its heaviest column is done: profiles/r05_engine_sort_ab.txt)
    g.sort_cols = !g.cols_mode && g.any_sim >= 0 && g.max_m <= 15000;  // (the sort's bins live in LDS)
    g.mix(g.sort_cols);
    size_t off = align_up(g.res_words * 4, 4096);
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off = align_up(off + bytes, 256);
        return at;
    };
    g.raw_base = off;
    for (int i = 0; i < K; ++i) g.lay[i].raw = take((size_t)c.m[items[i].k] * round_up(c.n[items[i].k], 64) + 256);
    g.raw_bytes = off - g.raw_base;
    for (int i = 0; i < K; ++i) {
        const int m = c.m[items[i].k], n = c.n[items[i].k];
        const size_t ld = round_up(n, 64), nchunk = (n + 31) / 32, m_pad = round_up(m, 128), ldw = round_up(m, 64);
        const size_t ncp = msak::bx_cols_pad(n), ldk = msak::bx_ldk(m);
        EngineLayout &y = g.lay[i];
        const EngineKind kind = items[i].kind;
        // RepresentativeTrimmer: planes and the pair pass; the identities land in the result region.  The gap statistics (and what
        // one more pass over the rows computes): the rows are all it needs on the device
        if (kind == ENGINE_REPRESENTATIVE || kind == ENGINE_SIMILARITY) y.planes = take(((size_t)msak::planes_total() * nchunk * m_pad + 64) * 4);
        if (kind == ENGINE_SIMILARITY) {
            y.ident = take(((size_t)m * ldw + 512) * 4);
            y.w = take(((size_t)m * ldw + 512) * 4);
            y.wlow = take((msak::bx_wlow_rows(m) + 2) * ldw * 4);
            y.wbar = take(((size_t)m + 128) * 4);
            y.row_avg = take(((size_t)m + 64) * 4);
            y.row_max = take(((size_t)m + 64) * 4);
            if (g.cols_mode) {
                y.codeR = take((size_t)m * ld + 256);
            } else {
                y.codeT = take(ncp * ldk + 64);
                y.off = take((ncp * ldk + 64) * 4);
                y.trow = take((ncp * ldk + 64) * 2);
                y.nvalid = take((ncp + 64) * 4);
            }
            y.simnum = take(((size_t)n + 64) * 4);
            y.simden = take(((size_t)n + 64) * 4);
            y.simstate = g.multi ? take(msak::lg_state_floats(n) * 4) : 0;
            y.cols = g.sort_cols ? take(((size_t)n + 64) * 4) : 0;  // (the wave-per-column kernel's columns by weight: sort_columns_batch)
        }
    }
    g.mix(g.multi);
    g.arena_bytes = off;
    return g;
}

// How the rows of every alignment of the group go up.  Rows the copy engine takes as they lie (page-locked, or 16-byte aligned
// rows of a multiple of 16 bytes) go up in a copy each -- 8 us of the copy queue per small alignment, beside the kernels of the
// group before; the others are packed into pinned staging at the same offsets (the calling thread and the idle workers) and go
// up in one copy per run.  (Packing everything small, measured: 1.7 ms of five threads per 25 MB of cache-cold rows against
// 2.1 ms of copy queue that nobody waits for.)
static void engine_row_routes(const BatchCall &c, const Engine *e, const std::vector<Engine::Item> &items, EngineGroup &g) {
    const int K = (int)items.size();
    g.packed.assign(K, 0);
    g.fetch.assign(K, nullptr);
    for (int i = 0; i < K; ++i) {
        const int k = items[i].k, m = c.m[k];
        const size_t ld = round_up(c.n[k], 64);
        const uint8_t *rows = c.data[k];
        const int64_t hld = c.ld[k];
        bool locked = false;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, rows) == hipSuccess) locked = at.type == hipMemoryTypeHost;
        else (void)hipGetLastError();
        const bool direct = hld == (int64_t)ld || (locked && hld % 8 == 0) || (hld % 16 == 0 && reinterpret_cast<uintptr_t>(rows) % 16 == 0);
        g.packed[i] = !direct;
        // small page-locked alignments: the device fetches the rows itself (one launch per group); big ones keep their copy
        // (one DMA transfer at the link's rate needs no help)
        if (locked && e->fetch_max_bytes > 0 && (size_t)m * ld <= (size_t)e->fetch_max_bytes) {
            void *dp = nullptr;
            if (hipHostGetDevicePointer(&dp, const_cast<uint8_t *>(rows), 0) == hipSuccess && dp) {
                g.fetch[i] = static_cast<const uint8_t *>(dp);
                g.packed[i] = 0;
            } else {
                (void)hipGetLastError();
            }
        }
    }
    g.any_packed = std::find(g.packed.begin(), g.packed.end(), 1) != g.packed.end();
}

// The descriptor tables of a group and the block prefix sums of its kernel families, into the host copy `h` of the metadata.
static void engine_tables(const BatchCall &c, const Engine::Lane &L, const EngineGroup &g, const EngineMeta &h) {
    const int K = (int)L.items.size();
    uint8_t *A = L.arena.p;
    int32_t *res_d = reinterpret_cast<int32_t *>(A);
    for (int f = 0; f < F_COUNT; ++f) h.pf[(size_t)f * (K + 1)] = 0;
    for (int i = 0; i < K; ++i) {
        const Engine::Item &it = L.items[i];
        const int k = it.k, m = c.m[k], n = c.n[k];
        const EngineLayout &y = g.lay[i];
        msak::BAlign d = {};
        d.raw = A + y.raw;
        d.fetch_src = g.fetch[i];
        d.fetch_ld = c.ld[k];
        d.ld = round_up(n, 64);
        d.ldk = msak::bx_ldk(m);
        d.planes = reinterpret_cast<uint32_t *>(A + y.planes);
        d.flags = res_d + it.res_word;
        d.gaps = d.flags + 16;
        d.indets = d.gaps + it.npad;
        d.rowtot = d.indets + it.npad;
        d.mdk = reinterpret_cast<float *>(d.rowtot + it.mpad);
        d.kind = it.kind;
        d.extra = res_d + it.extra_word;
        d.gated = it.kind == ENGINE_SIMILARITY && c.params[k].method == MSA_METHOD_AUTOMATED1;
        d.ident = d.gated ? reinterpret_cast<float *>(A + y.ident) : nullptr;
        d.w = reinterpret_cast<float *>(A + y.w);
        d.wlow = reinterpret_cast<float *>(A + y.wlow);
        if (it.kind == ENGINE_REPRESENTATIVE) d.ident = reinterpret_cast<float *>(d.extra), d.w = nullptr, d.wlow = nullptr;
        if (it.kind == ENGINE_OVERLAP) d.ov_need = static_cast<int>(std::ceil(c.params[k].residue_overlap * static_cast<float>(m - 1)));
        d.wbar = reinterpret_cast<float *>(A + y.wbar);
        d.row_avg = reinterpret_cast<float *>(A + y.row_avg);
        d.row_max = reinterpret_cast<float *>(A + y.row_max);
        d.codeT = A + y.codeT;
        d.codeR = A + y.codeR;
        d.off = reinterpret_cast<uint32_t *>(A + y.off);
        d.trow = reinterpret_cast<uint16_t *>(A + y.trow);
        d.nvalid = reinterpret_cast<int32_t *>(A + y.nvalid);
        d.simnum = reinterpret_cast<float *>(A + y.simnum);
        d.simden = reinterpret_cast<float *>(A + y.simden);
        d.m = m, d.n = n, d.nchunk = (n + 31) / 32, d.m_pad = round_up(m, 128), d.ldw = round_up(m, 64);
        d.ncols_pad = msak::bx_cols_pad(n);
        d.indet4 = 0x01010101u * c.indet[k];
        h.bt[i] = d;
        msak::LgAlign l = {};
        l.voff = d.off, l.vtrow = d.trow, l.nvalid = d.nvalid, l.codeT = d.codeT;
        l.wlow = d.wlow, l.wup = d.w, l.wbar = d.wbar, l.num_out = d.simnum, l.den_out = d.simden;
        l.state = g.multi ? reinterpret_cast<float *>(A + y.simstate) : nullptr;
        l.gate = d.gated ? d.flags + ST_GATE : nullptr;
        const bool sim = it.kind == ENGINE_SIMILARITY;
        // (only the alignments whose trim runs the similarity kernel: max_m -- the sort's LDS bins -- is taken over those)
        l.cols = g.sort_cols && sim ? reinterpret_cast<const int32_t *>(A + y.cols) : nullptr;
        l.ldk = d.ldk, l.m = m, l.n = n, l.ldw = d.ldw, l.ncols = n;
        h.lt[i] = l;
        auto add = [&](int f, int blocks) {
            const bool runs = sim || f <= F_ROWTOT || (it.kind == ENGINE_REPRESENTATIVE && (f == F_PLANES || f == F_PAIRS)) ||
                              (it.kind == ENGINE_OVERLAP && f == F_OVERLAP) || (it.kind == ENGINE_DIGESTS && f == F_DIGEST);
            h.pf[(size_t)f * (K + 1) + i + 1] = h.pf[(size_t)f * (K + 1) + i] + (runs ? blocks : 0);
        };
        add(F_FETCH, g.fetch[i] ? (int)(((int64_t)m * (d.ld / 16) + 255) / 256) : 0);
        add(F_GAPS, (int)((d.ld / 4 + 255) / 256) * ((m + 63) / 64));
        add(F_ROWTOT, (m + 3) / 4);
        add(F_PLANES, ((d.nchunk + 1) / 2) * ((d.m_pad + 255) / 256));
        add(F_PAIRS, msak::pair_tiles_pipe(m, d.m_pad));
        add(F_WMEANS, g.cols_mode ? 0 : (m + 64 + 3) / 4);  // (the predictor's input: the wave-per-column kernel only)
        add(F_IDROWS, d.gated ? (m + 3) / 4 : 0);
        add(F_ENCODE, g.cols_mode ? (int)((d.ld + 255) / 256) * ((m + 15) / 16) : (d.ncols_pad / 64) * (int)(d.ldk / 64));
        add(F_COMPACT, g.cols_mode ? 0 : (d.ncols_pad + 3) / 4);
        add(F_FINISH, (n + 255) / 256);
        add(F_COLS, g.cols_mode ? (n + 63) / 64 : n);
        add(F_OVERLAP, it.kind == ENGINE_OVERLAP ? (m + 3) / 4 : 0);
        add(F_DIGEST, it.kind == ENGINE_DIGESTS ? (m + 3) / 4 : 0);
    }
}

// The rows of the group into the arena on stream `st`: the packed ones through the staging buffer (one copy per run), the
// direct ones in a copy each; the fetched ones are the first kernel's (engine_launch).
static int engine_upload_rows(msa_batch *b, msa_ctx *tc, Engine::Lane &L, const EngineGroup &g, hipStream_t st) {
    const BatchCall &c = b->call;
    const int K = (int)L.items.size();
    uint8_t *A = L.arena.p;
    if (g.any_packed) {
        // pack (the calling thread and the idle workers), then one copy per run of packed alignments
        uint8_t *stage = L.h_stage.p;
        engine_parallel_for(b, K, [&](int32_t i, int) {
            if (!g.packed[i]) return;
            const int k = L.items[i].k, m = c.m[k], n = c.n[k];
            const size_t ld = round_up(n, 64);
            const uint8_t *rows = c.data[k];
            const int64_t hld = c.ld[k];
            uint8_t *dst = stage + (g.lay[i].raw - g.raw_base);
            for (int r = 0; r < m; ++r) {
                std::memcpy(dst + (size_t)r * ld, rows + (size_t)r * hld, (size_t)n);
                std::memset(dst + (size_t)r * ld + n, 0, ld - n);
            }
        });
    }
    for (int i = 0; i < K; ++i) {
        const int k = L.items[i].k, m = c.m[k], n = c.n[k];
        const size_t ld = round_up(n, 64);
        if (g.fetch[i]) continue;
        if (g.packed[i]) {
            int j = i;
            while (j + 1 < K && g.packed[j + 1]) ++j;
            const size_t from = g.lay[i].raw, to = j + 1 < K ? g.lay[j + 1].raw : g.raw_base + g.raw_bytes;
            HIPCHK(tc, hipMemcpyAsync(A + from, L.h_stage.p + (from - g.raw_base), to - from, hipMemcpyHostToDevice, st));
            i = j;
            continue;
        }
        const uint8_t *rows = c.data[k];
        const int64_t hld = c.ld[k];
        uint8_t *dst = A + g.lay[i].raw;
        if (hld == (int64_t)ld) HIPCHK(tc, hipMemcpyAsync(dst, rows, (size_t)m * ld, hipMemcpyHostToDevice, st));
        else HIPCHK(tc, hipMemcpy2DAsync(dst, ld, rows, (size_t)hld, (size_t)n, (size_t)m, hipMemcpyHostToDevice, st));
    }
    return MSA_OK;
}

// The launch sequence of a group -- one launch per kernel family on the lane's two queues -- and the one copy of its results
// back.  `h` / `d`: the metadata as the host and the device see it.
static int engine_launch(const BatchCall &c, msa_ctx *tc, Engine::Lane &L, const EngineGroup &g, const EngineMeta &h, const EngineMeta &d) {
    const int K = (int)L.items.size();
    auto PF = [&](int f) { return d.pf + (size_t)f * (K + 1); };
    auto NB = [&](int f) { return h.pf[(size_t)f * (K + 1) + K]; };
    hipStream_t st = L.pre;
    msak::launch_fetch_rows_batch(st, d.bt, PF(F_FETCH), K, NB(F_FETCH));
    msak::launch_gap_counts_batch(st, d.bt, PF(F_GAPS), K, NB(F_GAPS));
    if (g.sort_cols) msak::launch_sort_columns_batch(st, d.bt, d.lt, K, g.max_m);
    msak::launch_row_nongap_batch(st, d.bt, PF(F_ROWTOT), K, NB(F_ROWTOT));
    msak::launch_overlap_rows_batch(st, d.bt, PF(F_OVERLAP), K, NB(F_OVERLAP));
    msak::launch_row_digest_batch(st, d.bt, PF(F_DIGEST), K, NB(F_DIGEST));
    msak::launch_prep_planes_batch(st, d.bt, PF(F_PLANES), K, NB(F_PLANES));
    int min_nchunk = 1 << 30;
    for (const Engine::Item &it : L.items)
        if (it.kind == ENGINE_SIMILARITY || it.kind == ENGINE_REPRESENTATIVE) min_nchunk = std::min(min_nchunk, (c.n[it.k] + 31) / 32);
    msak::launch_pair_counts_batch(st, d.bt, PF(F_PAIRS), K, NB(F_PAIRS), min_nchunk);
    msak::launch_w_row_means_batch(st, d.bt, PF(F_WMEANS), K, NB(F_WMEANS));
    msak::launch_identity_stats_batch(st, d.bt, PF(F_IDROWS), K, NB(F_IDROWS));
    const int npos = g.any_sim >= 0 ? c.params[L.items[g.any_sim].k].npos : 0;
    if (g.cols_mode) msak::launch_sim_encode_rm_batch(st, d.bt, PF(F_ENCODE), K, NB(F_ENCODE), tc->lut.p);
    else msak::launch_sim_lists_batch(st, d.bt, PF(F_ENCODE), NB(F_ENCODE), PF(F_COMPACT), NB(F_COMPACT), K, tc->lut.p, npos);
    HIPCHK(tc, hipEventRecord(L.prepared, st));
    st = L.stream;
    HIPCHK(tc, hipStreamWaitEvent(st, L.prepared, 0));
    if (g.cols_mode) {
        msak::launch_similarity_cols_batch(st, d.bt, PF(F_COLS), K, NB(F_COLS), tc->tab.p);
    } else {
        int launches = 0;
        const int er = msak::launch_similarity_lg_batch(st, d.lt, PF(F_COLS), K, NB(F_COLS), g.max_m, npos, tc->tab.p, g.multi, &launches);
        if (er) return fail_hip(tc, (hipError_t)er, "launch_similarity (batch)");
    }
    msak::launch_sim_finish_batch(st, d.bt, PF(F_FINISH), K, NB(F_FINISH));
    HIPCHK(tc, hipGetLastError());
    HIPCHK(tc, hipMemcpyAsync(L.h_res.p, L.arena.p, g.res_words * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(tc, hipEventRecord(L.done, st));
    return MSA_OK;
}

// one group on lane L: layout, tables, uploads, launches; engine_finish waits for it
int engine_enqueue(msa_batch *b, Engine *e, Engine::Lane &L, const std::vector<Engine::Item> &group, int group_index) {
    const BatchCall &c = b->call;
    msa_ctx *tc = e->tables;
    const int K = (int)group.size();
    if (!L.stream) {
        int least = 0, greatest = 0;
        HIPCHK(tc, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(tc, hipStreamCreateWithPriority(&L.pre, hipStreamNonBlocking, greatest));
        HIPCHK(tc, hipStreamCreateWithPriority(&L.stream, hipStreamNonBlocking, least));
        HIPCHK(tc, hipEventCreateWithFlags(&L.prepared, hipEventDisableTiming));
        HIPCHK(tc, hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
    }
    L.items = group;
    EngineGroup g = engine_layout(c, e, L.items);
    engine_row_routes(c, e, L.items, g);
    for (int i = 0; i < K; ++i) {  // what was decided, for msa_batch_debug_routes
        const int k = L.items[i].k;
        const bool sim = L.items[i].kind == ENGINE_SIMILARITY;
        const int rows = g.fetch[i] ? MSA_ROUTE_ROWS_FETCHED
                         : g.packed[i] ? MSA_ROUTE_ROWS_PACKED
                         : c.ld[k] == (int64_t)round_up(c.n[k], 64) ? MSA_ROUTE_ROWS_LINEAR
                                                                    : MSA_ROUTE_ROWS_COPY_2D;
        b->routes[k] = MSA_ROUTE_ENGINE | (sim && g.cols_mode ? MSA_ROUTE_LANE_PER_COLUMN : 0) |
                       (sim && !g.cols_mode && g.multi ? MSA_ROUTE_SEVERAL_LAUNCHES : 0) | rows << MSA_ROUTE_ROWS_SHIFT |
                       group_index << MSA_ROUTE_GROUP_SHIFT;
    }
    HIPCHK(tc, L.arena.reserve(g.arena_bytes));
    g.mix((uint64_t)(uintptr_t)L.arena.p);
    const size_t meta_bytes = engine_meta_bytes(K);
    HIPCHK(tc, L.meta.reserve(meta_bytes));
    HIPCHK(tc, L.h_meta.reserve(meta_bytes));
    HIPCHK(tc, L.h_res.reserve(g.res_words * 4 + 64));
    if (g.any_packed) {
        // (the staging mirrors the raw region.  A grown staging buffer starts as zeros: the runs copied out of it span the slack
        // and the alignment gaps between the packed alignments, which only ever hold what the buffer held when it was allocated
        // -- the arena's padding stays zero whatever way the rows arrive)
        const size_t had = L.h_stage.cap;
        HIPCHK(tc, L.h_stage.reserve(g.raw_bytes));
        if (L.h_stage.cap != had) std::memset(L.h_stage.p, 0, L.h_stage.cap);
    }
    const EngineMeta h = engine_meta(L.h_meta.p, K), d = engine_meta(L.meta.p, K);
    engine_tables(c, L, g, h);
    hipStream_t st = L.pre;
    // zeroes: everything when the layout differs from the one the arena was last zeroed for (padding of W, of the rows:
    // the kernels write the same entries for the same layout), else the result region alone (counts, flags)
    if (g.sig != L.sig) {
        HIPCHK(tc, hipMemsetAsync(L.arena.p, 0, g.arena_bytes, st));
        L.sig = g.sig;
    } else {
        HIPCHK(tc, hipMemsetAsync(L.arena.p, 0, g.res_words * 4, st));
    }
    HIPCHK(tc, hipMemcpyAsync(L.meta.p, L.h_meta.p, meta_bytes, hipMemcpyHostToDevice, st));
    int rc = engine_upload_rows(b, tc, L, g, st);
    if (rc == MSA_OK) rc = engine_launch(c, tc, L, g, h, d);
    if (rc != MSA_OK) return rc;
    L.busy = true;
    return MSA_OK;
}

// The selection decisions of one alignment of a finished group, on view `v` (trim_impl reads the statistics the group's
// result copy brought back).
void engine_select_item(msa_batch *b, Engine::Lane &L, const Engine::Item &it, msa_ctx *v) {
    const BatchCall &c = b->call;
    int32_t *res = reinterpret_cast<int32_t *>(L.h_res.p);
    const int k = it.k, m = c.m[k], n = c.n[k];
    int32_t *flags = res + it.res_word;
    v->m = m, v->n = n, v->indet = c.indet[k], v->ld = round_up(n, 64);
    v->raw = L.arena.p;  // (never read through the view)
    v->host_rows = c.data[k], v->host_ld = c.ld[k];
    v->h_flags.p = flags;
    v->h_gaps.assign(flags + 16, flags + 16 + n);
    v->h_indets.assign(flags + 16 + it.npad, flags + 16 + it.npad + n);
    v->h_rowtot.p = flags + 16 + 2 * it.npad;
    v->rowtot_staged = 2;
    v->h_f32.p = reinterpret_cast<float *>(flags + 16 + 2 * it.npad + it.mpad);
    v->pairflag_state = 2;
    v->have_gaps = true;
    // what the trimmers that remove sequences read
    const int32_t *extra = res + it.extra_word;
    v->ov_valid = false;
    v->pref_ident = nullptr, v->pref_lengths = nullptr, v->pref_hashes = nullptr;
    if (it.kind == ENGINE_OVERLAP) {  // Cleaner::calculateSpuriousVector's values, as overlap() derives them from the counts
        v->ov_vals.resize(m);
        for (int i = 0; i < m; ++i) v->ov_vals[i] = static_cast<float>(extra[i]) / n;
        v->ov_key = c.params[k].residue_overlap;
        v->ov_valid = true;
        v->ov_colcnt = false;
    } else if (it.kind == ENGINE_REPRESENTATIVE) {
        v->pref_ident = reinterpret_cast<const float *>(extra);
        v->ldw = round_up(m, 64);
    } else if (it.kind == ENGINE_DIGESTS) {
        v->pref_lengths = extra;
        v->pref_hashes = reinterpret_cast<const unsigned long long *>(extra + it.mpad);
    }
    msa_trim_info local;
    msa_trim_info *info = c.info ? c.info + k : &local;
    const int rc = no_throw([&] { return trim_impl(v, c.params + k, c.keep_res[k], c.keep_seq[k], info); });
    if (rc == MSA_E_FALLBACK) {
        if (v->tuning.trace) std::fprintf(stderr, "[engine] alignment %d (%d x %d) needs the device again: ordinary context\n", k, m, n);
        std::lock_guard<std::mutex> lk(b->mu);
        b->sel_redo.push_back(k);
        b->routes[k] |= MSA_ROUTE_SELECTION_REDONE;
        return;
    }
    b->only_gaps[k] = v->only_gaps_rows;
    c.rc[k] = rc;
    b->sel_finished[k] = 1;
}

// items of the job in flight until none is left (the calling thread and every idle worker)
int engine_job_some(msa_batch *b, int thread) {
    int mine = 0;
    for (;;) {
        const int32_t i = b->sel_next.fetch_add(1, std::memory_order_relaxed);
        if (i >= b->sel_total) break;
        b->sel_fn(i, thread);
        ++mine;
    }
    return mine;
}

// fn(item, thread) for item = 0 .. total-1, by the calling thread and the workers that are idle; returns the calling thread's share
int engine_parallel_for(msa_batch *b, int32_t total, std::function<void(int32_t, int)> fn) {
    const bool share = total >= 8 && !b->workers.empty();
    {
        std::lock_guard<std::mutex> lk(b->mu);
        b->sel_fn = std::move(fn);
        b->sel_total = total;
        b->sel_next.store(0);
        if (share) {
            b->sel_open = true;
            ++b->sel_generation;
        }
    }
    if (share) b->cv_work.notify_all();
    const int mine = engine_job_some(b, (int)b->workers.size());
    if (share) {  // no helper joins from here on; wait for those that hold items
        std::unique_lock<std::mutex> lk(b->mu);
        b->sel_open = false;
        b->cv_done.wait(lk, [&] { return b->sel_active == 0; });
    }
    return mine;
}

// wait for a lane's group and take its selection decisions (with the workers that are idle: the host side of a trim is
// 10 - 20 us of cut points and masks per alignment, serial work that would otherwise leave the device waiting on batches of
// small alignments); alignments that need the device again are collected in b->sel_redo
int engine_finish(msa_batch *b, Engine *e, Engine::Lane &L) {
    if (!L.busy) return MSA_OK;
    L.busy = false;
    msa_ctx *tc = e->tables;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(tc, hipEventSynchronize(L.done));
    const auto t1 = std::chrono::steady_clock::now();
    const int mine = engine_parallel_for(b, (int32_t)L.items.size(), [&](int32_t i, int thread) { engine_select_item(b, L, L.items[i], e->views[thread]); });
    if (e->trace)
        std::fprintf(stderr, "[engine] group of %zu: waited %.0f us, selection %.0f us (%d of them by the calling thread)\n", L.items.size(),
                     std::chrono::duration<double, std::micro>(t1 - t0).count(),
                     std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count(), mine);
    return MSA_OK;
}

void engine_destroy(Engine *e) {
    if (!e) return;
    if (e->tables) (void)hipSetDevice(e->tables->device);
    for (Engine::Lane &L : e->lanes) {
        if (L.pre) (void)hipStreamSynchronize(L.pre);
        if (L.stream) (void)hipStreamSynchronize(L.stream);
        L.arena.release(), L.meta.release(), L.h_meta.release(), L.h_res.release(), L.h_stage.release();
        if (L.done) (void)hipEventDestroy(L.done);
        if (L.prepared) (void)hipEventDestroy(L.prepared);
        if (L.stream) (void)hipStreamDestroy(L.stream);
        if (L.pre) (void)hipStreamDestroy(L.pre);
    }
    for (msa_ctx *v : e->views) {  // (their pinned pointers are the lanes': nothing of their own to release)
        v->h_flags.p = nullptr, v->h_rowtot.p = nullptr, v->h_f32.p = nullptr;
        delete v;
    }
    if (e->tables) msa_ctx_destroy(e->tables);
    delete e;
}

// the engine's share of the call in flight (`share`, largest first), in groups, two groups in flight
int engine_run(msa_batch *b, const std::vector<Engine::Item> &share) {
    if (share.empty()) return MSA_OK;
    const BatchCall &c = b->call;
    if (!b->engine) {
        Engine *e = new (std::nothrow) Engine();
        if (!e) return MSA_E_NOMEM;
        int rc = msa_ctx_create(b->device, &e->tables);
        if (rc != MSA_OK) {
            delete e;
            return rc;
        }
        for (size_t w = 0; w <= b->workers.size(); ++w) {
            msa_ctx *v = new msa_ctx();
            v->device = b->device;
            v->tuning = e->tables->tuning;
            v->prefetched = true;
            e->views.push_back(v);
        }
        e->trace = std::getenv("MSA_TRACE") != nullptr;
        if (msak::diagnostics_enabled())
            if (const char *ev = std::getenv("MSA_BATCH_COLS_MAX")) e->cols_max_m = std::min(128, std::atoi(ev));  // (the kernel's LDS tile)
        b->engine = e;
    }
    Engine *e = b->engine;
    msa_ctx *tc = e->tables;
    HIPCHK(tc, hipSetDevice(b->device));
    TuneScope tune(tc);
    int rc = MSA_OK;
    for (const Engine::Item &it : share)
        if (it.kind == ENGINE_SIMILARITY) {  // the one set of tables of the call (engine_takes: every such alignment shares it)
            const msa_trim_params *p0 = c.params + it.k;
            tc->indet = c.indet[it.k];
            if ((rc = ensure_tables(tc, p0->vhash, p0->dist, p0->npos))) return rc;
            break;
        }
    // groups: about a quarter of the call each (at least two groups in flight whenever there are two alignments), bounded
    // by the arena (~8 GB) and by 256 alignments
    const int total = (int)share.size();
    int parts = 4;
    const int target = std::max(1, std::min(256, (total + parts - 1) / parts));
    std::vector<std::vector<Engine::Item>> groups;
    {
        std::vector<Engine::Item> cur;
        double bytes = 0;
        for (const Engine::Item &it : share) {
            const int m = c.m[it.k], n = c.n[it.k];
            const double need = (double)m * m * 12 + (double)msak::bx_cols_pad(n) * msak::bx_ldk(m) * 7 + (double)m * n * 2;
            // (a group is small alignments -- a lane per column -- or not: the kernels differ)
            const bool turn = !cur.empty() && (c.m[cur.front().k] <= e->cols_max_m) != (m <= e->cols_max_m);
            if (!cur.empty() && ((int)cur.size() >= target || bytes + need > 8e9 || turn)) {
                groups.push_back(cur);
                cur.clear();
                bytes = 0;
            }
            cur.push_back(it);
            bytes += need;
        }
        if (!cur.empty()) groups.push_back(cur);
    }
    b->sel_redo.clear();
    b->sel_finished.assign((size_t)c.count, 0);
    const int G = (int)groups.size();
    int first_error = MSA_OK;
    for (int g = 0; g < G && first_error == MSA_OK; ++g) {
        Engine::Lane &L = e->lanes[g % e->nlanes];
        rc = engine_finish(b, e, L);  // (the group that used this lane `nlanes` steps ago)
        const auto te = std::chrono::steady_clock::now();
        if (rc == MSA_OK) rc = engine_enqueue(b, e, L, groups[g], g);
        if (e->trace)
            std::fprintf(stderr, "[engine] group %d enqueued in %.0f us\n", g,
                         std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - te).count());
        if (rc != MSA_OK) first_error = rc;
    }
    for (int g = 0; g < e->nlanes; ++g) {
        rc = engine_finish(b, e, e->lanes[(G + g) % e->nlanes]);
        if (rc != MSA_OK && first_error == MSA_OK) first_error = rc;
    }
    if (first_error != MSA_OK) {
        for (Engine::Lane &L : e->lanes) {
            if (L.pre) (void)hipStreamSynchronize(L.pre);
            if (L.stream) (void)hipStreamSynchronize(L.stream);
            L.busy = false;
        }
        for (const Engine::Item &it : share)
            if (!b->sel_finished[it.k]) c.rc[it.k] = first_error;  // (the groups that were through keep their results)
        return first_error;
    }
    // the selection of these needs another pass over the rows: an ordinary context
    for (int32_t k : b->sel_redo) c.rc[k] = rows_item(b, tc, k);
    return MSA_OK;
}

// Splits the call's alignments (`order`: all of them, largest first) into what the engine takes (batched kernels, the calling
// thread; returned) and what the workers take (a context per alignment; left in `order`).
static std::vector<Engine::Item> engine_share(msa_batch *b, std::vector<int32_t> &order) {
    const BatchCall &c = b->call;
    std::vector<Engine::Item> share;
    std::vector<int32_t> rest;
    const msa_trim_params *ref = nullptr;
    for (int32_t k : order) {
        const EngineKind kind = engine_takes(b, k, ref);
        if (kind == ENGINE_NONE) {
            rest.push_back(k);
            continue;
        }
        if (!ref && kind == ENGINE_SIMILARITY) ref = c.params + k;
        share.push_back(Engine::Item{k, kind, 0, 0, 0, 0});
    }
    // A handful of small alignments is faster through the worker contexts (each a compact pipeline of three launches,
    // compact_begin) than as a group of the batched kernels with its arena, tables and ten launches: 8 x (100 x 1000) 0.31
    // against 0.96 ms, 16: 0.57 / 1.11, 32: 1.0 / 1.2, 64: 2.0 / 1.45 (tools/small_batch.py).
    if ((int)share.size() < b->engine_min_count) {
        for (const Engine::Item &it : share) rest.push_back(it.k);
        std::stable_sort(rest.begin(), rest.end(), [&](int32_t x, int32_t y) {
            return (double)c.m[x] * c.m[x] * c.n[x] > (double)c.m[y] * c.m[y] * c.n[y];
        });
        share.clear();
    }
    order.swap(rest);
    return share;
}

// the index into params_by_type of a detected sequence type (SequenceTypes bits): amino acids and an undetected type 0,
// nucleotides 1, degenerate nucleotides 2 -- the matrices the Python side picks by type (trimmer.type_index)
static int seq_type_index(uint32_t ty) { return (ty & 4) || ty == 0 ? 0 : (ty & 8) ? 2 : 1; }

// one text of a TEXTS call on worker context ctx: parse, trim with the parameters of its type, names (and rows, and the text)
int fasta_item(msa_batch *b, msa_ctx *ctx, int32_t k) {
    const BatchCall &c = b->call;
    msa_batch::FastaResult &r = b->fasta[k];
    ctx->only_gaps_rows.clear();
    r.parse_rc = msa_upload_fasta(ctx, c.texts[k], c.lens[k], c.valid, &r.info, &r.detail);
    const int m = r.info.m, n = r.info.n;
    auto names = [&] {  // the records' names, as (offset, length) into the text
        r.name_off.resize((size_t)m);
        r.name_len.resize((size_t)m);
        return msa_text_names(ctx, r.name_off.data(), r.name_len.data());
    };
    if (r.parse_rc != MSA_OK) {  // (a failure names its record: the names came with the parse)
        if ((r.parse_rc == MSA_E_BAD_RESIDUE || r.parse_rc == MSA_E_LENGTH_MISMATCH) && m > 0 && names() != MSA_OK) r.name_off.clear(), r.name_len.clear();
        return r.parse_rc;
    }
    r.keep_res.assign((size_t)n, 1);
    r.keep_seq.assign((size_t)m, 1);
    int rc = MSA_OK;
    if (m > 0 && n > 0) {  // (an empty alignment never reaches the device: trim_batch)
        rc = msa_trim(ctx, c.params_by_type + seq_type_index(r.info.seq_type), r.keep_res.data(), r.keep_seq.data(), &r.tinfo);
        b->only_gaps[k] = ctx->only_gaps_rows;
        if (rc == MSA_OK && c.want_rows) {
            r.rows.resize((size_t)m * n);
            rc = msa_download_rows(ctx, r.rows.data(), n);
        }
        if (rc == MSA_OK && c.emit_format >= 0) {  // the trimmed text, composed under the masks of this trim with the text's own names
            int64_t len = 0;
            const int erc = msa_emit_text(ctx, c.emit_format, r.keep_res.data(), r.keep_seq.data(), nullptr, nullptr, nullptr, &len, &r.text_flags);
            if (erc == MSA_OK && !r.text_flags) {
                r.text.reset(new uint8_t[(size_t)std::max<int64_t>(len, 1)]);
                if ((rc = msa_download_text(ctx, r.text.get(), len)) == MSA_OK) r.text_len = len;
                else r.text.reset();
            } else if (erc != MSA_OK && !(r.text_flags & MSA_TEXT_F_TOO_LONG)) {
                rc = erc;  // (a text too long for the device is the caller's to write: the flag says so, the trim stands)
            }
        }
    }
    if (rc == MSA_OK && m > 0) rc = names();
    return rc;
}

void batch_worker(msa_batch *b, int w) {
    (void)hipSetDevice(b->device);
    uint64_t seen = 0, seen_sel = 0;
    for (;;) {
        bool select = false;
        {
            std::unique_lock<std::mutex> lk(b->mu);
            b->cv_work.wait(lk, [&] { return b->stop || b->generation != seen || b->sel_generation != seen_sel; });
            if (b->stop) return;
            if (b->generation != seen) {
                seen = b->generation;
            } else {
                seen_sel = b->sel_generation;
                if (!b->sel_open) continue;  // (the job was over before this thread woke up)
                select = true;
                ++b->sel_active;
            }
        }
        if (select) {  // the engine's selection step: a helper beside the calling thread
            engine_job_some(b, w);
            std::lock_guard<std::mutex> lk(b->mu);
            if (--b->sel_active == 0) b->cv_done.notify_all();
            continue;
        }
        const BatchCall &c = b->call;
        msa_ctx *ctx = b->ctxs[w];
        for (;;) {
            const int32_t slot = b->next.fetch_add(1, std::memory_order_relaxed);
            if (slot >= (int32_t)b->order.size()) break;
            const int32_t k = b->order[slot];
            const int rc = no_throw([&] { return c.kind == BatchCall::TEXTS ? fasta_item(b, ctx, k) : rows_item(b, ctx, k); });
            if (rc == MSA_E_NOMEM || rc == MSA_E_INVALID) {
                if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
                (void)hipStreamSynchronize(ctx->stream);
                ctx->upload_pending = false;
            }
            c.rc[k] = rc;
        }
        {
            std::lock_guard<std::mutex> lk(b->mu);
            if (--b->running == 0) b->cv_done.notify_all();
        }
    }
}

// The protocol of every call, of either kind: refuse a second call, take `call`, order its alignments largest first (`key`),
// hand the workers their share, run the engine's share (ROWS only) on the calling thread, wait for the workers, clear the
// call, return the first failure.
template <class Key>
static int run_call(msa_batch *b, const BatchCall &call, Key key) {
    const int32_t count = call.count;
    if (count == 0) return MSA_OK;
    const bool rows = call.kind == BatchCall::ROWS;
    std::vector<Engine::Item> share;
    {
        std::unique_lock<std::mutex> lk(b->mu);
        if (b->running || b->in_call) return MSA_E_INVALID;  // one call at a time per batch object
        b->in_call = true;
        b->call = call;
        // largest first: the last alignments to finish are the small ones
        b->order.resize(count);
        for (int32_t k = 0; k < count; ++k) b->order[k] = k;
        std::stable_sort(b->order.begin(), b->order.end(), [&](int32_t x, int32_t y) { return key(x) > key(y); });
        if (rows && b->use_engine) share = engine_share(b, b->order);
        // what the last call left behind goes now (msa_batch_fasta_result, msa_batch_only_gaps_rows: results of the last call only)
        b->only_gaps.assign(count, {});
        b->fasta.clear();
        if (!rows) b->fasta.resize((size_t)count);
        b->routes.assign(rows ? (size_t)count : 0, 0);
        for (int32_t k = 0; k < count; ++k) call.rc[k] = MSA_OK;
        b->next.store(0);
        b->running = b->order.empty() ? 0 : (int)b->workers.size();
        if (b->running) ++b->generation;
    }
    if (!b->order.empty()) b->cv_work.notify_all();
    const auto t_call = std::chrono::steady_clock::now();
    const int engine_rc = no_throw([&] { return engine_run(b, share); });
    if (engine_rc != MSA_OK)
        for (const Engine::Item &it : share)
            if (call.rc[it.k] == MSA_OK && !(it.k < (int32_t)b->sel_finished.size() && b->sel_finished[it.k])) call.rc[it.k] = engine_rc;
    {
        std::unique_lock<std::mutex> lk(b->mu);
        b->cv_done.wait(lk, [&] { return b->running == 0; });
        b->in_call = false;
        b->call = BatchCall();
    }
    if (rows && std::getenv("MSA_TRACE"))
        std::fprintf(stderr, "[msa_trim_batch] %d alignments: %zu through the batched kernels, %zu through the workers, %.2f ms\n", (int)count,
                     share.size(), b->order.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count());
    for (int32_t k = 0; k < count; ++k)
        if (call.rc[k] != MSA_OK) return call.rc[k];
    return MSA_OK;
}
}  // namespace msai

extern "C" {

int msa_batch_create(int device, int32_t workers, msa_batch **out) {
    if (!out || workers < 1 || workers > 64) return MSA_E_INVALID;
    *out = nullptr;
    msa_batch *b = new (std::nothrow) msa_batch();
    if (!b) return MSA_E_NOMEM;
    b->device = device;
    if (msak::diagnostics_enabled()) {  // (MSA_DIAGNOSTICS: msastat_kernels.hip)
        if (const char *e = std::getenv("MSA_BATCH_ENGINE")) b->use_engine = std::atoi(e) != 0;
        if (const char *e = std::getenv("MSA_BATCH_ENGINE_MAX")) b->engine_max_work = std::atof(e);
        if (const char *e = std::getenv("MSA_BATCH_ENGINE_MIN")) b->engine_min_count = std::atoi(e);
    }
    for (int w = 0; w < workers; ++w) {
        msa_ctx *c = nullptr;
        const int rc = msa_ctx_create(device, &c);
        if (rc != MSA_OK) {
            for (msa_ctx *x : b->ctxs) msa_ctx_destroy(x);
            delete b;
            return rc;
        }
        b->ctxs.push_back(c);
    }
    for (int w = 0; w < workers; ++w) b->workers.emplace_back(batch_worker, b, w);
    *out = b;
    return MSA_OK;
}

void msa_batch_destroy(msa_batch *b) {
    if (!b) return;
    {
        std::lock_guard<std::mutex> lk(b->mu);
        b->stop = true;
    }
    b->cv_work.notify_all();
    for (std::thread &t : b->workers) t.join();
    for (msa_ctx *c : b->ctxs) msa_ctx_destroy(c);
    engine_destroy(b->engine);
    delete b;
}

int32_t msa_batch_workers(const msa_batch *b) { return b ? (int32_t)b->workers.size() : 0; }

int msa_trim_batch(msa_batch *b, int32_t count, const uint8_t *const *data, const int32_t *m, const int32_t *n, const int64_t *ld,
                   const uint8_t *indet, const msa_trim_params *params, uint8_t *const *keep_res, uint8_t *const *keep_seq,
                   msa_trim_info *info, int32_t *rc) {
    if (!b || count < 0 || (count > 0 && (!data || !m || !n || !ld || !indet || !params || !keep_res || !keep_seq || !rc)))
        return MSA_E_INVALID;
    BatchCall call;
    call.kind = BatchCall::ROWS, call.count = count, call.rc = rc;
    call.data = data, call.m = m, call.n = n, call.ld = ld, call.indet = indet, call.params = params;
    call.keep_res = keep_res, call.keep_seq = keep_seq, call.info = info;
    return run_call(b, call, [&](int32_t k) { return (double)m[k] * m[k] * n[k]; });  // (cost ~ m^2 n)
}

static int trim_batch_fasta(msa_batch *b, int32_t count, const uint8_t *const *texts, const int64_t *lens, const uint8_t *valid,
                            const msa_trim_params params_by_type[3], int32_t want_rows, int32_t format, int32_t *rc) {
    if (!b || count < 0 || (count > 0 && (!texts || !lens || !params_by_type || !rc))) return MSA_E_INVALID;
    BatchCall call;
    call.kind = BatchCall::TEXTS, call.count = count, call.rc = rc;
    call.texts = texts, call.lens = lens, call.valid = valid, call.params_by_type = params_by_type;
    call.want_rows = want_rows != 0, call.emit_format = format;
    return run_call(b, call, [&](int32_t k) { return lens[k]; });
}

int msa_trim_batch_fasta(msa_batch *b, int32_t count, const uint8_t *const *texts, const int64_t *lens, const uint8_t *valid,
                         const msa_trim_params params_by_type[3], int32_t want_rows, int32_t *rc) {
    return trim_batch_fasta(b, count, texts, lens, valid, params_by_type, want_rows, -1, rc);
}

int msa_trim_batch_fasta_emit(msa_batch *b, int32_t count, const uint8_t *const *texts, const int64_t *lens, const uint8_t *valid,
                              const msa_trim_params params_by_type[3], int32_t want_rows, int32_t format, int32_t *rc) {
    if (!msai::text_format_known(format)) return MSA_E_INVALID;
    return trim_batch_fasta(b, count, texts, lens, valid, params_by_type, want_rows, format, rc);
}

int msa_batch_fasta_text(msa_batch *b, int32_t k, const uint8_t **text, int64_t *len, uint32_t *flags) {
    if (!b || k < 0 || k >= (int32_t)b->fasta.size()) return MSA_E_INVALID;
    const msa_batch::FastaResult &r = b->fasta[k];
    if (text) *text = r.text_len >= 0 ? r.text.get() : nullptr;
    if (len) *len = r.text_len;
    if (flags) *flags = r.text_flags;
    return MSA_OK;
}

int msa_batch_fasta_result(msa_batch *b, int32_t k, msa_text_info *info, const uint8_t **keep_res, const uint8_t **keep_seq,
                           const int64_t **name_off, const int32_t **name_len, const uint8_t **rows, msa_trim_info *tinfo,
                           msa_err_detail *detail) {
    if (!b || k < 0 || k >= (int32_t)b->fasta.size()) return MSA_E_INVALID;
    const msa_batch::FastaResult &r = b->fasta[k];
    if (info) *info = r.info;
    if (keep_res) *keep_res = r.keep_res.data();
    if (keep_seq) *keep_seq = r.keep_seq.data();
    if (name_off) *name_off = r.name_off.data();
    if (name_len) *name_len = r.name_len.data();
    if (rows) *rows = r.rows.empty() ? nullptr : r.rows.data();
    if (tinfo) *tinfo = r.tinfo;
    if (detail) *detail = r.detail;
    return r.parse_rc;
}

int msa_batch_only_gaps_rows(msa_batch *b, int32_t k, int32_t *rows, int32_t cap) {
    if (!b || k < 0 || k >= (int32_t)b->only_gaps.size() || cap < 0 || (!rows && cap > 0)) return MSA_E_INVALID;
    const std::vector<int32_t> &v = b->only_gaps[k];
    std::copy_n(v.begin(), std::min((int)v.size(), (int)cap), rows);
    return (int)v.size();
}

int msa_batch_debug_routes(msa_batch *b, int32_t *route, int32_t cap) {
    if (!b || cap < 0 || (!route && cap > 0)) return MSA_E_INVALID;
    std::lock_guard<std::mutex> lk(b->mu);
    if (b->in_call) return MSA_E_INVALID;
    std::copy_n(b->routes.begin(), std::min((int)b->routes.size(), (int)cap), route);
    return (int)b->routes.size();
}

const char *msa_batch_last_hip_error(const msa_batch *b, int32_t worker) {
    return (b && worker >= 0 && worker < (int32_t)b->ctxs.size()) ? b->ctxs[worker]->hip_err : "";
}

}  // extern "C"
