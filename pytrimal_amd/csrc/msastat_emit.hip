// msastat_emit.hip -- the context's residue matrix + masks + names -> the text of the trimmed alignment in device memory
// (msa_text_size, msa_emit_text, msa_download_text of include/msastat.h): the bytes pytrimal_amd's host writers produce
// (alignment.py: _fast_fasta, _fast_clustal, _write_phylip40, _write_phylip32, _write_phylippaml), without host rows.
//
// All layouts are closed forms of the kept counts and the kept names' lengths.  With km kept sequences, kn kept columns,
// L_i the bytes of kept name i that reach the text and R = kn + ceil(kn / 60) (a record's residues and line ends):
//   FASTA    record i starts at P_i + i * R with P_i = sum_{j<i} (2 + L_j); it is '>' name '\n', then R bytes in which every 61st
//            (and the last) is '\n';
//   Clustal  37 header bytes, then blocks of B = km * (W + 61) + 2 bytes (the last one shorter), W = max L_i + 5: km lines of
//            name, blanks up to W, the block's residues, '\n', and two '\n' behind them.
// The PHYLIP family: H header bytes " km kn\n", W = max(max L_i, 10) + 3, nb = max(ceil(kn / 60), 1) blocks of c_b = min(60,
// kn - 60 b) columns, a line's residues in groups of ten joined by one blank: g(c) = c + ceil(c / 10) - 1 bytes (g(0) = 0);
//   PHYLIP40    per block km lines of W + g(c_b) + 1 bytes (the name in block 0 only, blanks up to W, the groups, '\n'), then '\n';
//   PHYLIP32    per sequence its nb lines, then '\n': records of S = sum_b (W + g(c_b) + 1) + 1 bytes, record i at H + i * S;
//   PHYLIPPAML  per sequence one line of W + kn + 1 bytes: the name, blanks up to W, all residues ungrouped, '\n'.
// Two passes, none of which waits for another workgroup:
//   emit_index_kernel     one workgroup: exclusive scans of the two masks -> the kept-column and kept-row lists; over the kept
//                         rows a scan of 2 + L_i -> P_i, the longest name, and whether a kept name holds a byte >= 0x80 (the
//                         host writer counts characters there, the caller takes it instead);
//   emit_fasta_kernel /   output-driven: a lane owns 16 consecutive bytes of the text, finds its record (a binary search over
//   emit_clustal_kernel / the record starts) or block and line (two divisions; PHYLIP's records are uniform) once, then walks:
//   emit_phylip_kernel    every byte is '>' / ' ' / '\n', a header or name byte, or raw[row * ld + col[k]]; one aligned
//                         16-byte store per lane, no atomics.
// Work per byte does not depend on the line length or on how many columns the masks dropped.  Positions in the text are 32-bit
// (a text of 2^31 bytes or more is refused before the second pass), offsets into the matrix 64-bit.
#include "msastat_ctx.h"

namespace {

constexpr int ET = 1024;        // threads of the index pass's one workgroup
constexpr int CT = 256;         // threads per workgroup of the compose pass
constexpr int EB = 16;          // bytes of the text per lane
constexpr int LINE = 60;        // residues per line, both formats
constexpr int CLUSTAL_HEAD = 37;
__device__ const char CLUSTAL_HEAD_TEXT[CLUSTAL_HEAD + 1] = "CLUSTAL multiple sequence alignment\n\n";
constexpr int FASTA_M10 = 10;
constexpr int GROUP = 10;       // PHYLIP: residues per group
constexpr int PHYLIP_HEAD = 24; // the longest header, " 2147483647 2147483647\n", fits
constexpr int PHYLIP_MINW = 10, PHYLIP_PAD = 3;
enum { P40 = 0, P32 = 1, PAML = 2 };  // the PHYLIP layouts

enum { ES_KM = 0, ES_KN = 1, ES_NAMES = 2 /* sum of 2 + L_i */, ES_MAXL = 3, ES_FLAG = 4, ES_WORDS = 8 };

struct IndexArgs {
    const uint8_t *keep_res, *keep_seq;
    int n, m;
    const uint8_t *nbase;  // name i: nbase[noff[i] ...], nlen[i] bytes (or up to nend[i] when nlen is null)
    const uint32_t *noff, *nend;
    const int32_t *nlen;
    int cap;               // bytes of a name that reach the text
    long long *pre;        // [m + 1]
    int32_t *cols, *rows, *nlenk;
    long long *stats;      // ES_WORDS
};

struct ComposeArgs {
    const uint8_t *raw;
    long long ld;
    const uint8_t *nbase;
    const uint32_t *noff;
    const long long *pre;
    const int32_t *cols, *rows, *nlenk;
    int km, kn;
    int width;        // Clustal: the name column
    uint32_t total;   // bytes of the text (< 2^31)
    uint8_t *out;     // writable up to the next multiple of 16
};

struct PhylipArgs {
    ComposeArgs c;                // width: W
    uint8_t head[PHYLIP_HEAD];    // the header line, formatted on the host
    int hlen;
};

// exclusive scan of one value per thread over the workgroup; *total = the sum (sh: ET words)
__device__ long long block_scan(long long v, long long *sh, long long *total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < ET; d <<= 1) {
        const long long x = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const long long incl = sh[t];
    *total = sh[ET - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(ET) void emit_index_kernel(IndexArgs a) {
    __shared__ long long sh[ET];
    __shared__ int s_max, s_flag;
    const int t = threadIdx.x;
    if (t == 0) s_max = 0, s_flag = 0;  // (the first scan's barriers lie between this and the atomics below)
    long long total;
    {  // kept columns: every thread a run of consecutive columns
        const long long per = ((long long)a.n + ET - 1) / ET;
        const long long c0 = min((long long)a.n, t * per), c1 = min((long long)a.n, c0 + per);
        int cnt = 0;
        for (long long c = c0; c < c1; ++c) cnt += a.keep_res[c] != 0;
        long long at = block_scan(cnt, sh, &total);
        for (long long c = c0; c < c1; ++c)
            if (a.keep_res[c]) a.cols[at++] = (int32_t)c;
        if (t == 0) a.stats[ES_KN] = total;
    }
    {  // kept rows, their names
        const long long per = ((long long)a.m + ET - 1) / ET;
        const long long r0 = min((long long)a.m, t * per), r1 = min((long long)a.m, r0 + per);
        int cnt = 0, mx = 0;
        long long bytes = 0;
        bool bad = false;
        for (long long r = r0; r < r1; ++r) {
            if (!a.keep_seq[r]) continue;
            const int L = a.nlen ? a.nlen[r] : (int)(a.nend[r] - a.noff[r]);
            const uint8_t *p = a.nbase + a.noff[r];
            for (int b = 0; b < L; ++b) bad |= p[b] >= 0x80;
            mx = max(mx, L);
            bytes += 2 + min(L, a.cap);
            ++cnt;
        }
        if (mx) atomicMax(&s_max, mx);
        if (bad) atomicOr(&s_flag, 1);
        long long km;
        long long at = block_scan(cnt, sh, &km);
        long long pos = block_scan(bytes, sh, &total);
        for (long long r = r0; r < r1; ++r) {
            if (!a.keep_seq[r]) continue;
            const int L = a.nlen ? a.nlen[r] : (int)(a.nend[r] - a.noff[r]);
            const int Lc = min(L, a.cap);
            a.rows[at] = (int32_t)r;
            a.nlenk[at] = Lc;
            a.pre[at] = pos;
            pos += 2 + Lc;
            ++at;
        }
        if (t == 0) {  // (s_max, s_flag: complete since the barriers of the two scans)
            a.pre[km] = total;
            a.stats[ES_KM] = km;
            a.stats[ES_NAMES] = total;
            a.stats[ES_MAXL] = s_max;
            a.stats[ES_FLAG] = s_flag;
        }
    }
}

__device__ __forceinline__ void put(uint32_t (&w)[4], int j, uint32_t c) { w[j >> 2] |= c << ((j & 3) * 8); }

__global__ __launch_bounds__(CT) void emit_fasta_kernel(ComposeArgs a) {
    const uint32_t pos0 = (blockIdx.x * (uint32_t)CT + threadIdx.x) * (uint32_t)EB;
    if (pos0 >= a.total) return;
    const uint32_t kn = (uint32_t)a.kn;
    const uint32_t R = kn + (kn + LINE - 1) / LINE;
    int lo = 0, hi = a.km - 1;  // the record of the lane's first byte: the last one that starts at or before it
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((unsigned long long)a.pre[mid] + (unsigned long long)mid * R <= pos0) lo = mid;
        else hi = mid - 1;
    }
    int i = lo;
    uint32_t o = pos0 - (uint32_t)((unsigned long long)a.pre[i] + (unsigned long long)i * R);
    uint32_t L = (uint32_t)a.nlenk[i];
    int row = a.rows[i];
    const uint8_t *name = a.nbase + a.noff[row];
    const uint8_t *src = a.raw + (size_t)row * (size_t)a.ld;
    uint32_t w[4] = {0, 0, 0, 0};
    const int cnt = (int)min((uint32_t)EB, a.total - pos0);
#pragma unroll
    for (int j = 0; j < EB; ++j) {
        if (j >= cnt) continue;
        if (o == 2 + L + R) {  // the next record (every record has its two bytes: pos0 + j < total keeps i < km)
            ++i;
            o = 0;
            L = (uint32_t)a.nlenk[i];
            row = a.rows[i];
            name = a.nbase + a.noff[row];
            src = a.raw + (size_t)row * (size_t)a.ld;
        }
        uint32_t c;
        if (o == 0) c = '>';
        else if (o <= L) c = name[o - 1];
        else if (o == L + 1) c = '\n';
        else {
            const uint32_t q = o - (L + 2), line = q / (LINE + 1), r = q - line * (LINE + 1), k = line * LINE + r;
            c = (r == LINE || k == kn) ? (uint32_t)'\n' : (uint32_t)src[a.cols[k]];
        }
        put(w, j, c);
        ++o;
    }
    *reinterpret_cast<uint4 *>(a.out + pos0) = make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(CT) void emit_clustal_kernel(ComposeArgs a) {
    const uint32_t pos0 = (blockIdx.x * (uint32_t)CT + threadIdx.x) * (uint32_t)EB;
    if (pos0 >= a.total) return;
    const uint32_t km = (uint32_t)a.km, kn = (uint32_t)a.kn, W = (uint32_t)a.width;
    const uint32_t nb = (kn + LINE - 1) / LINE, B = km * (W + LINE + 1) + 2;
    // the walk's state behind the header: block b of cb columns and lines of Lb bytes, line i (km: the two line ends behind the
    // block), byte j of it
    uint32_t b = 0, i = 0, j = 0, cb = 0, Lb = 0, cur = 0xffffffffu, L = 0;
    const uint8_t *name = nullptr, *src = nullptr;
    bool placed = false;
    uint32_t w[4] = {0, 0, 0, 0};
    const int cnt = (int)min((uint32_t)EB, a.total - pos0);
#pragma unroll
    for (int x = 0; x < EB; ++x) {
        if (x >= cnt) continue;
        const uint32_t p = pos0 + x;
        if (p < CLUSTAL_HEAD) {
            put(w, x, (uint32_t)CLUSTAL_HEAD_TEXT[p]);
            continue;
        }
        if (!placed) {  // (p < total behind the header: there is a block, km and kn are not 0)
            const uint32_t q = p - CLUSTAL_HEAD;
            b = min(q / B, nb - 1);
            const uint32_t off = q - b * B;
            cb = min((uint32_t)LINE, kn - LINE * b);
            Lb = W + cb + 1;
            if (off >= km * Lb) i = km, j = off - km * Lb;
            else i = off / Lb, j = off - i * Lb;
            placed = true;
        }
        uint32_t c;
        if (i == km) {
            c = '\n';
            if (++j == 2) {
                ++b, i = 0, j = 0;
                cb = min((uint32_t)LINE, kn - LINE * b);  // (not read behind the last block)
                Lb = W + cb + 1;
            }
        } else {
            if (i != cur) {
                cur = i;
                L = (uint32_t)a.nlenk[i];
                const int row = a.rows[i];
                name = a.nbase + a.noff[row];
                src = a.raw + (size_t)row * (size_t)a.ld;
            }
            if (j < W) c = j < L ? (uint32_t)name[j] : (uint32_t)' ';
            else if (j == W + cb) c = '\n';
            else c = src[a.cols[b * LINE + (j - W)]];
            if (++j == Lb) ++i, j = 0;
        }
        put(w, x, c);
    }
    *reinterpret_cast<uint4 *>(a.out + pos0) = make_uint4(w[0], w[1], w[2], w[3]);
}

// bytes of a PHYLIP line's residue part: c residues in groups of ten joined by one blank
__host__ __device__ __forceinline__ uint32_t grouped(uint32_t c) { return c ? c + (c + GROUP - 1) / GROUP - 1 : 0; }

template <int LAYOUT>
__global__ __launch_bounds__(CT) void emit_phylip_kernel(PhylipArgs pa) {
    const ComposeArgs &a = pa.c;
    const uint32_t pos0 = (blockIdx.x * (uint32_t)CT + threadIdx.x) * (uint32_t)EB;
    if (pos0 >= a.total) return;
    const uint32_t km = (uint32_t)a.km, kn = (uint32_t)a.kn, W = (uint32_t)a.width, H = (uint32_t)pa.hlen;
    const uint32_t nb = LAYOUT == PAML ? 1u : max((kn + LINE - 1) / LINE, 1u);
    const uint32_t LF = W + grouped(LINE) + 1;  // a line of a full block
    // columns of block b (0 behind the last one, where nothing is read) and the bytes of its lines
    auto columns = [&](uint32_t b) { return LAYOUT == PAML ? kn : (LINE * b < kn ? min((uint32_t)LINE, kn - LINE * b) : 0u); };
    auto line_bytes = [&](uint32_t c) { return W + (LAYOUT == PAML ? c : grouped(c)) + 1; };
    // the walk's state behind the header: block b, sequence i, byte j of its line of Lb bytes; term: the '\n' behind a block
    // (P40) or behind a sequence's lines (P32) comes next
    uint32_t b = 0, i = 0, j = 0, Lb = 0, cur = 0xffffffffu, L = 0;
    bool term = false, placed = false;
    const uint8_t *name = nullptr, *src = nullptr;
    uint32_t w[4] = {0, 0, 0, 0};
    const int cnt = (int)min((uint32_t)EB, a.total - pos0);
#pragma unroll
    for (int x = 0; x < EB; ++x) {
        if (x >= cnt) continue;
        const uint32_t p = pos0 + x;
        if (p < H) {
            put(w, x, (uint32_t)pa.head[p]);
            continue;
        }
        if (!placed) {  // (every divisor is a part of the text that exists, so it is below 2^31; km == 0: P40's one '\n')
            const uint32_t q = p - H;
            if (LAYOUT == P40) {
                b = nb > 1 ? min(q / (km * LF + 1), nb - 1) : 0u;
                const uint32_t off = q - b * (km * LF + 1);
                Lb = line_bytes(columns(b));
                if (off >= km * Lb) term = true;
                else i = off / Lb, j = off - i * Lb;
            } else if (LAYOUT == P32) {
                const uint32_t S = (nb - 1) * LF + line_bytes(columns(nb - 1)) + 1;
                i = q / S;
                const uint32_t off = q - i * S;
                if (off == S - 1) term = true;
                else b = min(off / LF, nb - 1), j = off - b * LF;
                Lb = line_bytes(columns(b));
            } else {
                Lb = line_bytes(kn);
                i = q / Lb, j = q - i * Lb;
            }
            placed = true;
        }
        uint32_t c;
        if (term) {
            c = '\n';
            term = false, j = 0;
            if (LAYOUT == P40) ++b, i = 0;
            else ++i, b = 0;
            Lb = line_bytes(columns(b));
        } else {
            if (i != cur) {
                cur = i;
                L = (uint32_t)a.nlenk[i];
                const int row = a.rows[i];
                name = a.nbase + a.noff[row];
                src = a.raw + (size_t)row * (size_t)a.ld;
            }
            if (j < W) c = (b == 0 && j < L) ? (uint32_t)name[j] : (uint32_t)' ';
            else if (j == Lb - 1) c = '\n';
            else if (LAYOUT == PAML) c = src[a.cols[j - W]];
            else {
                const uint32_t r = j - W, grp = r / (GROUP + 1), at = r - grp * (GROUP + 1);
                c = at == GROUP ? (uint32_t)' ' : (uint32_t)src[a.cols[b * LINE + grp * GROUP + at]];
            }
            if (++j == Lb) {
                j = 0;
                if (LAYOUT == P40) term = ++i == km;
                else if (LAYOUT == P32) term = ++b == nb, Lb = line_bytes(columns(b));
                else ++i;
            }
        }
        put(w, x, c);
    }
    *reinterpret_cast<uint4 *>(a.out + pos0) = make_uint4(w[0], w[1], w[2], w[3]);
}

bool is_m10(int format) {
    return format == MSA_TEXT_FASTA_M10 || format == MSA_TEXT_PHYLIP40_M10 || format == MSA_TEXT_PHYLIP32_M10 || format == MSA_TEXT_PHYLIPPAML_M10;
}
bool is_phylip(int format) { return format >= MSA_TEXT_PHYLIP40 && format <= MSA_TEXT_PHYLIPPAML_M10; }
int phylip_layout(int format) { return (format - MSA_TEXT_PHYLIP40) / 2; }

// PHYLIP's header line " km kn\n" (kn printed as 0 without sequences, as the host writer does) -> its length
int phylip_head(char (&out)[PHYLIP_HEAD + 1], int64_t km, int64_t kn) {
    return std::snprintf(out, sizeof out, " %lld %lld\n", (long long)km, (long long)(km ? kn : 0));
}

// the text's length from the kept counts, sum (2 + L_i) and max L_i, both with the cut to 10 applied (saturates at INT64_MAX)
int64_t text_total(int format, int64_t km, int64_t kn, int64_t names_bytes, int64_t max_len) {
    unsigned __int128 t;
    if (is_phylip(format)) {
        using u128 = unsigned __int128;
        char head[PHYLIP_HEAD + 1];
        if (km == 0) kn = 0;
        const u128 H = (u128)phylip_head(head, km, kn), W = (u128)std::max<int64_t>(max_len, PHYLIP_MINW) + PHYLIP_PAD;
        const int64_t full = kn / LINE, rest = kn % LINE, nb = std::max<int64_t>(full + (rest != 0), 1);
        // a sequence's lines over all blocks: nb names or paddings and line ends, the residues, their blanks
        const u128 lines = (u128)nb * (W + 1) + (u128)kn + (u128)full * (grouped(LINE) - LINE) + (u128)(grouped((uint32_t)rest) - (uint32_t)rest);
        const int layout = phylip_layout(format);
        if (layout == P40) t = H + (u128)km * lines + (u128)nb;
        else if (layout == P32) t = H + (u128)km * (lines + 1);
        else t = H + (u128)km * (W + (u128)kn + 1);
    } else if (format == MSA_TEXT_CLUSTAL) {
        if (km == 0 || kn == 0) return CLUSTAL_HEAD;
        const unsigned __int128 nb = (unsigned __int128)((kn + LINE - 1) / LINE);
        t = (unsigned __int128)CLUSTAL_HEAD + nb * 2 + (unsigned __int128)km * (nb * (unsigned __int128)(max_len + 5 + 1) + (unsigned __int128)kn);
    } else {
        t = (unsigned __int128)names_bytes + (unsigned __int128)km * (unsigned __int128)(kn + (kn + LINE - 1) / LINE);
    }
    return t > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)t;
}

size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

using namespace msai;

extern "C" {

int msa_text_size(int32_t format, int32_t kept_m, int32_t kept_n, const int32_t *name_len, int64_t *out) {
    if (!out || !text_format_known(format) || kept_m < 0 || kept_n < 0 || (kept_m > 0 && !name_len)) return MSA_E_INVALID;
    int64_t bytes = 0, mx = 0;
    for (int32_t i = 0; i < kept_m; ++i) {
        if (name_len[i] < 0) return MSA_E_INVALID;
        const int64_t L = is_m10(format) ? std::min<int64_t>(name_len[i], FASTA_M10) : name_len[i];
        bytes += 2 + L;
        mx = std::max(mx, L);
    }
    *out = text_total(format, kept_m, kept_n, bytes, mx);
    return MSA_OK;
}

int msa_emit_text(msa_ctx *c, int32_t format, const uint8_t *keep_res, const uint8_t *keep_seq, const uint8_t *names,
                  const int64_t *name_off, const int32_t *name_len, int64_t *len_out, uint32_t *flags_out) {
    if (!c || !len_out || !text_format_known(format)) return MSA_E_INVALID;
    *len_out = 0;
    if (flags_out) *flags_out = 0;
    c->em_len = -1;
    const int m = c->m, n = c->n;
    const bool own_names = names != nullptr || (m > 0 && (name_off || name_len));
    if (own_names) {
        if (m > 0 && (!names || !name_off || !name_len)) return MSA_E_INVALID;
    } else if (c->paths[0] != MSA_PATH_UPLOAD_FASTA || c->fa_m != m) {
        return MSA_E_INVALID;  // the alignment is not the last msa_upload_fasta's text: there are no names of it here
    }
    if (c->prefetched || (!c->raw && (int64_t)m * n > 0)) return MSA_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    // staging and its device image: [result words][noff m][nlen m][keep_res n][keep_seq m][name bytes]
    size_t names_bytes = 0;
    if (own_names)
        for (int i = 0; i < m; ++i) {
            if (name_off[i] < 0 || name_len[i] < 0) return MSA_E_INVALID;
            names_bytes = std::max(names_bytes, (size_t)name_off[i] + (size_t)name_len[i]);
        }
    if (names_bytes > (size_t)UINT32_MAX) return MSA_E_INVALID;
    const size_t o_stats = 0, o_noff = ES_WORDS * sizeof(long long), o_nlen = o_noff + (size_t)4 * m, o_res = o_nlen + (size_t)4 * m;
    const size_t o_seq = o_res + (size_t)n, o_names = up16(o_seq + (size_t)m), in_bytes = o_names + names_bytes + 16;
    HIPCHK(c, c->h_em.reserve(in_bytes));
    HIPCHK(c, c->em_in.reserve(in_bytes));
    uint8_t *h = c->h_em.p, *d = c->em_in.p;
    if (keep_res) std::memcpy(h + o_res, keep_res, (size_t)n);
    else std::memset(h + o_res, 1, (size_t)n);
    if (keep_seq) std::memcpy(h + o_seq, keep_seq, (size_t)m);
    else std::memset(h + o_seq, 1, (size_t)m);
    size_t up_from = o_res;
    if (own_names) {
        uint32_t *hoff = reinterpret_cast<uint32_t *>(h + o_noff);
        int32_t *hlen = reinterpret_cast<int32_t *>(h + o_nlen);
        for (int i = 0; i < m; ++i) hoff[i] = (uint32_t)name_off[i], hlen[i] = name_len[i];
        if (names_bytes) std::memcpy(h + o_names, names, names_bytes);
        up_from = o_noff;
    }
    const size_t up_to = own_names ? o_names + names_bytes : o_seq + (size_t)m;
    if (up_to > up_from) HIPCHK(c, hipMemcpyAsync(d + up_from, h + up_from, up_to - up_from, hipMemcpyHostToDevice, c->stream));
    // the index pass's lists: [pre m + 1][result words][cols n][rows m][nlenk m]
    const size_t i_stats = sizeof(long long) * ((size_t)m + 1), i_cols = i_stats + ES_WORDS * sizeof(long long), i_rows = i_cols + (size_t)4 * n;
    const size_t i_nlen = i_rows + (size_t)4 * m, idx_bytes = i_nlen + (size_t)4 * m + 16;
    HIPCHK(c, c->em_idx.reserve(idx_bytes));
    uint8_t *x = c->em_idx.p;
    IndexArgs ia;
    ia.keep_res = d + o_res, ia.keep_seq = d + o_seq, ia.n = n, ia.m = m;
    if (own_names) {
        ia.nbase = d + o_names, ia.noff = reinterpret_cast<const uint32_t *>(d + o_noff), ia.nend = nullptr;
        ia.nlen = reinterpret_cast<const int32_t *>(d + o_nlen);
    } else {
        ia.nbase = c->fa_text.p, ia.noff = c->fa_names.p, ia.nend = c->fa_names.p + m, ia.nlen = nullptr;
    }
    ia.cap = is_m10(format) ? FASTA_M10 : INT32_MAX;
    ia.pre = reinterpret_cast<long long *>(x), ia.stats = reinterpret_cast<long long *>(x + i_stats);
    ia.cols = reinterpret_cast<int32_t *>(x + i_cols), ia.rows = reinterpret_cast<int32_t *>(x + i_rows);
    ia.nlenk = reinterpret_cast<int32_t *>(x + i_nlen);
    emit_index_kernel<<<1, ET, 0, c->stream>>>(ia);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h + o_stats, ia.stats, ES_WORDS * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    SYNC(c);
    const long long *st = reinterpret_cast<const long long *>(h + o_stats);
    const int64_t km = st[ES_KM], kn = st[ES_KN];
    if (st[ES_FLAG]) {
        if (flags_out) *flags_out |= MSA_TEXT_F_NON_ASCII;
        return MSA_OK;
    }
    const int64_t max_len = std::min<int64_t>(st[ES_MAXL], ia.cap);  // (the index pass takes the longest name before the cut)
    const int64_t total = text_total(format, km, kn, st[ES_NAMES], max_len);
    if (total > (int64_t)INT32_MAX) {
        if (flags_out) *flags_out |= MSA_TEXT_F_TOO_LONG;
        return MSA_E_INVALID;
    }
    if (total > 0) {
        HIPCHK(c, c->em_out.reserve(up16((size_t)total) + 64));
        ComposeArgs ca;
        ca.raw = c->raw, ca.ld = c->ld, ca.nbase = ia.nbase, ca.noff = ia.noff, ca.pre = ia.pre, ca.cols = ia.cols, ca.rows = ia.rows;
        ca.nlenk = ia.nlenk, ca.km = (int)km, ca.kn = (int)kn, ca.width = (int)max_len + 5, ca.total = (uint32_t)total, ca.out = c->em_out.p;
        const unsigned grid = (unsigned)(((size_t)total + (size_t)CT * EB - 1) / ((size_t)CT * EB));
        if (is_phylip(format)) {
            PhylipArgs pa;
            char head[PHYLIP_HEAD + 1] = {};
            pa.c = ca, pa.c.kn = km ? (int)kn : 0, pa.c.width = (int)std::max<int64_t>(max_len, PHYLIP_MINW) + PHYLIP_PAD;
            pa.hlen = phylip_head(head, km, kn);
            std::memcpy(pa.head, head, PHYLIP_HEAD);
            const int layout = phylip_layout(format);
            if (layout == P40) emit_phylip_kernel<P40><<<grid, CT, 0, c->stream>>>(pa);
            else if (layout == P32) emit_phylip_kernel<P32><<<grid, CT, 0, c->stream>>>(pa);
            else emit_phylip_kernel<PAML><<<grid, CT, 0, c->stream>>>(pa);
        } else if (format == MSA_TEXT_CLUSTAL) emit_clustal_kernel<<<grid, CT, 0, c->stream>>>(ca);
        else emit_fasta_kernel<<<grid, CT, 0, c->stream>>>(ca);
        HIPCHK(c, hipGetLastError());
        if (std::getenv("MSA_TRACE"))
            std::fprintf(stderr, "[msa_emit_text] format %d: %lld x %lld kept of %d x %d, %lld bytes, %u workgroups\n", (int)format, (long long)km,
                         (long long)kn, m, n, (long long)total, grid);
    }
    c->em_len = total;
    *len_out = total;
    return MSA_OK;
}

int msa_download_text(msa_ctx *c, uint8_t *out, int64_t cap) {
    if (!c || c->em_len < 0 || cap < c->em_len || (!out && c->em_len > 0)) return MSA_E_INVALID;
    if (c->em_len == 0) return MSA_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->em_out.p, (size_t)c->em_len, hipMemcpyDeviceToHost, c->stream));
    SYNC(c);
    return MSA_OK;
}

}  // extern "C"
