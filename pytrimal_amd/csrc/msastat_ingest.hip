// msastat_ingest.hip -- FASTA text in device memory -> the context's residue matrix (msa_upload_fasta, msastat_ctx.hip).
//
// The host reader (msa_fasta_fill, msastat_host.cpp) is a state machine over the bytes: every byte moves the state of its line
// (start / header before the name / in the name / behind the name / sequence) and the counts of the current record.  Here the
// same machine runs as a scan.  A 16-byte chunk is summarised as a function of the line state it is entered in (five entries:
// line state after it, headers in it, residues before its first header and behind its last one, the length of its first whole
// record, the same two residue counts for letters), and these summaries compose associatively.  Three passes, none of which
// waits for another workgroup:
//   fasta_reduce_kernel   a workgroup per tile of 4096 bytes: the tile's summary (chunk summaries composed in an LDS tree);
//   fasta_scan_kernel     one workgroup: the summaries of all tiles composed in order -> the concrete state at every tile start,
//                         m (headers) and n (residues of the first record);
//   fasta_scatter_kernel  a workgroup per tile again: the state at every chunk start (down-sweep of concrete states), then each
//                         lane walks its 16 bytes: residue -> raw[record * ld + column], the record's name start / end, the
//                         first failure in stream order (one 32-bit atomicMin over byte offsets), the per-row counts of
//                         detect_alignment_type (first 100 letters).
// Work per byte is constant whatever the line length.  Offsets are 32-bit: texts of up to 2^31 - 1 bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "msastat.h"
#include "msastat_kernels.h"

namespace msak {
namespace {

constexpr int FT = 256;          // threads per workgroup
constexpr int FCHUNK = 16;       // bytes per lane (one 16-byte load)
static_assert(FASTA_TILE == FT * FCHUNK, "tile = workgroup x chunk");

// line states of the host walk
enum { LS_START = 0, LS_NAME0 = 1 /* header, blanks behind '>' */, LS_NAME = 2, LS_REST = 3 /* header behind the name */, LS_SEQ = 4, NLS = 5 };

// what a segment does when entered in one line state
struct Part {
    int L;            // line state behind the segment
    int h;            // header lines that start in it
    int pre, post;    // residues before its first header / behind its last one (both = all of them when h == 0)
    int len1;         // residues between its first and second header (h >= 2)
    int lpre, lpost;  // the same two counts for letters (bytes other than - . ?)
};
struct Fn {
    Part f[NLS];
};
struct St {  // concrete state at a byte offset
    int L, H, C, LC;  // line state, headers so far, residues of the current record, letters of it
};

__device__ __forceinline__ bool fa_blank(uint32_t c) { return c == ' ' || c == '\t' || c == '\r' || c == 11 || c == 12; }

__device__ __forceinline__ void part_step(Part &p, uint32_t c, int letter) {
    if (c == '\n') {
        p.L = LS_START;
        return;
    }
    if (fa_blank(c)) {
        if (p.L == LS_NAME) p.L = LS_REST;
        return;
    }
    int L = p.L;
    if (L == LS_START) {
        if (c == '>') {
            if (p.h == 1) p.len1 = p.post;
            ++p.h;
            p.post = 0;
            p.lpost = 0;
            p.L = LS_NAME0;
            return;
        }
        p.L = L = LS_SEQ;
    }
    if (L == LS_SEQ) {
        if (p.h == 0) {
            ++p.pre;
            p.lpre += letter;
        }
        ++p.post;
        p.lpost += letter;
    } else if (L == LS_NAME0) {
        p.L = LS_NAME;
    }
}

__device__ __forceinline__ Part part_then(const Part &a, const Part &b) {
    Part r;
    r.L = b.L;
    r.h = a.h + b.h;
    r.pre = a.h ? a.pre : a.pre + b.pre;
    r.lpre = a.h ? a.lpre : a.lpre + b.lpre;
    r.post = b.h ? b.post : a.post + b.pre;
    r.lpost = b.h ? b.lpost : a.lpost + b.lpre;
    r.len1 = a.h >= 2 ? a.len1 : (a.h == 1 ? (b.h ? a.post + b.pre : 0) : (b.h >= 2 ? b.len1 : 0));
    return r;
}

__device__ __forceinline__ const Part &part_at(const Fn &b, int L) {
    return b.f[L];
}

__device__ __forceinline__ Fn compose(const Fn &a, const Fn &b) {
    Fn r;
#pragma unroll
    for (int i = 0; i < NLS; ++i) r.f[i] = part_then(a.f[i], part_at(b, a.f[i].L));
    return r;
}

__device__ __forceinline__ Fn fn_identity() {
    Fn r;
#pragma unroll
    for (int i = 0; i < NLS; ++i) r.f[i] = Part{i, 0, 0, 0, 0, 0, 0};
    return r;
}

__device__ __forceinline__ St apply(const Fn &F, St s) {
    const Part &p = part_at(F, s.L);
    s.L = p.L;
    s.C = p.h ? p.post : s.C + p.pre;
    s.LC = p.h ? p.lpost : s.LC + p.lpre;
    s.H += p.h;
    return s;
}

__device__ __forceinline__ uint32_t byte_of(const uint4 &v, int j) {
    const uint32_t w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
    return (w >> ((j & 3) * 8)) & 0xffu;
}

// summary of the chunk at `base` (bytes beyond len are not part of the text)
__device__ __forceinline__ Fn chunk_fn(const uint8_t *text, int len, int64_t base, const uint8_t *cls) {
    Fn f = fn_identity();
    if (base < len) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + base);
        const int cnt = (int)min((int64_t)FCHUNK, len - base);
#pragma unroll
        for (int j = 0; j < FCHUNK; ++j) {
            if (j < cnt) {
                const uint32_t c = byte_of(v, j);
                const int letter = cls[c] & 1;
#pragma unroll
                for (int i = 0; i < NLS; ++i) part_step(f.f[i], c, letter);
            }
        }
    }
    return f;
}

// in-place up-sweep over FT summaries: sh[FT - 1] = the composition of all, sh[i] = left subtrees where the down-sweep needs them
__device__ void upsweep(Fn *sh) {
    const int tid = threadIdx.x;
    for (int d = 1; d < FT; d <<= 1) {
        __syncthreads();
        if (((tid + 1) & (2 * d - 1)) == 0) sh[tid] = compose(sh[tid - d], sh[tid]);
    }
    __syncthreads();
}

// concrete state at the start of every lane's chunk, from the state at the start of the whole range
__device__ St downsweep(const Fn *sh, St *st, St s0) {
    const int tid = threadIdx.x;
    if (tid == FT - 1) st[FT - 1] = s0;
    for (int d = FT / 2; d >= 1; d >>= 1) {
        __syncthreads();
        if (((tid + 1) & (2 * d - 1)) == 0) {
            const St s = st[tid];
            st[tid - d] = s;
            st[tid] = apply(sh[tid - d], s);
        }
    }
    __syncthreads();
    return st[tid];
}

__global__ __launch_bounds__(FT) void fasta_reduce_kernel(const uint8_t *__restrict__ text, int len, Fn *__restrict__ tilesum,
                                                          const uint8_t *__restrict__ tables) {
    __shared__ Fn sh[FT];
    __shared__ uint8_t cls[256];
    const int tid = threadIdx.x;
    cls[tid] = tables[256 + tid];
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * FASTA_TILE + tid * FCHUNK;  // (64-bit: the last tile of a text near 2^31 bytes)
    sh[tid] = chunk_fn(text, len, base, cls);
    upsweep(sh);
    if (tid == FT - 1) tilesum[blockIdx.x] = sh[FT - 1];
}

// one workgroup: every lane composes a run of tiles, the runs are scanned, every lane then writes its tiles' start states
__global__ __launch_bounds__(FT) void fasta_scan_kernel(const Fn *__restrict__ tilesum, int nt, St *__restrict__ tilestate,
                                                        int32_t *__restrict__ aux) {
    __shared__ Fn sh[FT];
    __shared__ St st[FT];
    const int tid = threadIdx.x;
    const int per = (nt + FT - 1) / FT;
    const int t0 = min(nt, tid * per), t1 = min(nt, t0 + per);
    Fn f = fn_identity();
    for (int t = t0; t < t1; ++t) f = compose(f, tilesum[t]);
    sh[tid] = f;
    upsweep(sh);
    const Part total = sh[FT - 1].f[LS_START];
    St s = downsweep(sh, st, St{LS_START, 0, 0, 0});
    for (int t = t0; t < t1; ++t) {
        tilestate[t] = s;
        s = apply(tilesum[t], s);
    }
    if (tid == 0) {
        aux[FA_M] = total.h;
        aux[FA_N] = total.h >= 2 ? total.len1 : (total.h == 1 ? total.post : 0);
        aux[FA_ERRKEY] = -1;  // 0xffffffff as an unsigned key: no failure
        for (int k = FA_KIND; k < FA_WORDS; ++k) aux[k] = 0;
    }
}

// DETAIL: one workgroup over the tile that holds the failure aux[FA_ERRKEY]: writes its (code, row, col, byte), nothing else
template <bool DETAIL>
__global__ __launch_bounds__(FT) void fasta_scatter_kernel(FastaArgs a, int tile0) {
    __shared__ Fn sh[FT];
    __shared__ St st[FT];
    __shared__ uint8_t valid[256], cls[256];
    const int tid = threadIdx.x;
    valid[tid] = a.tables[tid];
    cls[tid] = a.tables[256 + tid];
    __syncthreads();
    const int t = tile0 + blockIdx.x;
    const int len = a.len;
    const int64_t base = (int64_t)t * FASTA_TILE + tid * FCHUNK;
    sh[tid] = chunk_fn(a.text, len, base, cls);
    upsweep(sh);
    St s = downsweep(sh, st, static_cast<const St *>(a.tilestate)[t]);
    if (base >= len) return;
    const int n = a.aux[FA_N];
    const uint32_t key = static_cast<uint32_t>(a.aux[FA_ERRKEY]);
    auto fail = [&](uint32_t at, int code, int row, int col, int byte) {
        if (!DETAIL) {
            atomicMin(reinterpret_cast<unsigned int *>(a.aux + FA_ERRKEY), at);
        } else if (at == key) {
            a.aux[FA_KIND] = code, a.aux[FA_ROW] = row, a.aux[FA_COL] = col, a.aux[FA_BYTE] = byte;
        }
    };
    int cur_row = -1;
    unsigned long long acc = 0;  // the lane's type counts of row cur_row: letters, DNA, RNA, degenerate (16 bits each)
    const uint4 v = *reinterpret_cast<const uint4 *>(a.text + base);
    const int cnt = (int)min((int64_t)FCHUNK, len - base);
#pragma unroll
    for (int j = 0; j < FCHUNK; ++j) {
        if (j >= cnt) continue;
        const uint32_t c = byte_of(v, j);
        const int p = (int)base + j;  // (< len)
        if (c == '\n') {
            if (!DETAIL && s.L == LS_NAME0) a.name_off[s.H - 1] = p;
            if (!DETAIL && (s.L == LS_NAME0 || s.L == LS_NAME)) a.name_end[s.H - 1] = p;
            s.L = LS_START;
            continue;
        }
        if (fa_blank(c)) {
            if (s.L == LS_NAME) {
                if (!DETAIL) a.name_end[s.H - 1] = p;
                s.L = LS_REST;
            }
            continue;
        }
        if (s.L == LS_START) {
            if (c == '>') {
                if (s.H >= 1 && s.C != n) fail(p, MSA_E_LENGTH_MISMATCH, s.H - 1, s.C, 0);
                ++s.H;
                s.C = s.LC = 0;
                s.L = LS_NAME0;
                continue;
            }
            s.L = LS_SEQ;
        }
        if (s.L == LS_SEQ) {
            const int k = cls[c];
            if (s.H >= 1) {
                const int row = s.H - 1;
                if (s.C < n) {
                    if (!valid[c]) fail(p, MSA_E_BAD_RESIDUE, row, s.C, (int)c);
                    else if (!DETAIL) a.raw[(size_t)row * (size_t)a.ld + s.C] = (uint8_t)c;
                }
                if (!DETAIL && (k & 1) && s.LC < 100) {
                    if (row != cur_row) {
                        if (cur_row >= 0) atomicAdd(a.rowtype + cur_row, acc);
                        cur_row = row;
                        acc = 0;
                    }
                    acc += 1ull | ((unsigned long long)((k >> 1) & 1) << 16) | ((unsigned long long)((k >> 2) & 1) << 32) |
                           ((unsigned long long)((k >> 3) & 1) << 48);
                }
            }
            ++s.C;
            s.LC += k & 1;
        } else if (s.L == LS_NAME0) {
            if (!DETAIL) a.name_off[s.H - 1] = p;
            s.L = LS_NAME;
        }
    }
    if (!DETAIL && cur_row >= 0) atomicAdd(a.rowtype + cur_row, acc);
    if (len - base <= FCHUNK) {  // the lane of the last byte: the end of the text closes the last record and its name
        if (s.H >= 1 && s.C != n) fail((uint32_t)len, MSA_E_LENGTH_MISMATCH, s.H - 1, s.C, 0);
        if (!DETAIL && s.L == LS_NAME0) a.name_off[s.H - 1] = len;
        if (!DETAIL && (s.L == LS_NAME0 || s.L == LS_NAME)) a.name_end[s.H - 1] = len;
    }
}

// detect_alignment_type (pytrimal_amd/alignment.py) from the per-row counts: one wave-wide ballot per rule and row block
__global__ __launch_bounds__(FT) void fasta_type_kernel(const unsigned long long *__restrict__ rowtype, int m, int32_t *__restrict__ aux) {
    const int r = blockIdx.x * FT + threadIdx.x;
    bool protein = false, g_rna = false, g_dna = false, e_rna = false, e_dna = false;
    if (r < m) {
        const unsigned long long x = rowtype[r];
        const int k = (int)(x & 0xffff), hd = (int)((x >> 16) & 0xffff), hr = (int)((x >> 32) & 0xffff), dg = (int)(x >> 48);
        if (k > 0) {
            // (the float32 quotient against the DOUBLE literal 0.7, as upstream and the host rule compare it)
            const float kf = (float)k;
            protein = (double)__fdiv_rn((float)(hd + dg), kf) < 0.7 && (double)__fdiv_rn((float)(hr + dg), kf) < 0.7;
            g_rna = hr > hd && dg == 0;
            g_dna = hr < hd && dg == 0;
            e_rna = hr > hd && dg != 0;
            e_dna = hr < hd && dg != 0;
        }
    }
    const bool flags[5] = {protein, g_rna, g_dna, e_rna, e_dna};
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const unsigned long long b = __ballot(flags[i]);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(aux + FA_TYPES + i, (int)__popcll(b));
    }
}

}  // namespace

// (in 64 bits: len may be 2^31 - 1)
static int fasta_tiles(int len) { return (int)(((int64_t)len + FASTA_TILE - 1) / FASTA_TILE); }

size_t fasta_tile_sum_bytes() { return sizeof(Fn); }
size_t fasta_tile_state_bytes() { return sizeof(St); }

void launch_fasta_parse(hipStream_t s, const uint8_t *text, int len, void *tilesum, void *tilestate, const uint8_t *tables, int32_t *aux) {
    const int nt = fasta_tiles(len);
    fasta_reduce_kernel<<<nt, FT, 0, s>>>(text, len, static_cast<Fn *>(tilesum), tables);
    fasta_scan_kernel<<<1, FT, 0, s>>>(static_cast<const Fn *>(tilesum), nt, static_cast<St *>(tilestate), aux);
}

void launch_fasta_scatter(hipStream_t s, const FastaArgs &a) {
    const int nt = fasta_tiles(a.len);
    fasta_scatter_kernel<false><<<nt, FT, 0, s>>>(a, 0);
}

void launch_fasta_type(hipStream_t s, const unsigned long long *rowtype, int m, int32_t *aux) {
    if (m > 0) fasta_type_kernel<<<(m + FT - 1) / FT, FT, 0, s>>>(rowtype, m, aux);
}

void launch_fasta_detail(hipStream_t s, const FastaArgs &a, uint32_t key) {
    const int nt = fasta_tiles(a.len);
    const int tile = key >= (uint32_t)a.len ? nt - 1 : (int)(key / FASTA_TILE);
    fasta_scatter_kernel<true><<<1, FT, 0, s>>>(a, tile);
}

}  // namespace msak
