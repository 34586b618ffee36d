// pc_discover.hip -- the k-mer census behind adapter discovery: what is on the ends of the reads?
//
// kmer_count_kernel: every k-mer of every window adds 1 to a dense uint32[4^k] table.  A k-mer's code holds 2 bits per
// base, the first base in the highest bits, in SeqAn's Dna order (A 0, C 1, G 2, T/U 3, either case -- the byte -> code
// table of the scans, seqan/basic/alphabet_residue_tabs.h:113-140); a k-mer that covers any other byte (Dna5 'N') is
// not counted.  The kernel only adds: one table takes block after block of a streamed file, the caller zeroes it.
//
// Shape.  A wave takes one window (grid-stride over the windows) and walks it in chunks of kChunk = 256 k-mer starts,
// i.e. 256 + k - 1 bytes.  The chunk comes from HBM once, as ALIGNED dwords (a window may start at any byte: the dword
// below its first byte and the one that holds its last byte are fetched whole -- never a byte outside an aligned dword
// that holds a byte of the window), adjacent lanes on adjacent dwords.  The bytes are coded (0..3, 4 = not a base)
// and staged in the wave's own LDS strip, shifted so that the chunk's first base is byte 0.  Lane l then takes the four
// starts 4 l .. 4 l + 3: the 16 codes from 4 l on (4 + k - 1 <= 16) become one 32-bit word of sixteen 2-bit fields and
// a 16-bit mask of non-bases; start t's k-mer is (word << 2 t) >> (32 - 2 k), valid when bits t .. t + k - 1 of the
// mask are clear and the k-mer ends inside the window.  One no-return atomic add per valid k-mer.
//
// The kernel is bound by those atomics, not by bytes: a million 8-kb reads are 300 MB of end windows and about 280 M
// adds, and the adds are skewed -- every read that carries the adapter hits the same two dozen counters.  Equal codes
// are NOT merged inside the wave: what the skew costs on this chip is the open measurement of DESIGN.md section 13
// (tools/kmer_count_rate.py).
//
// kmer_select_kernel: the table entries with count >= min_count, appended to a capped list through one cursor.  A wave
// draws its slots with ONE returning atomic (ballot + popcount), so a threshold that most of a 4^12 table passes costs
// 260 k cursor updates, not 16 M.  The cursor counts every qualifying entry whether or not it fitted.
//
// insert_code_kernel (barcode discovery): the bases behind an aligned anchor as one code per window; described where it stands.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pc_kernels.h"

namespace pck {

namespace {

constexpr int kChunk = 256;                    // k-mer starts per chunk: four per lane
constexpr int kStrip = kChunk + 16;            // staged codes per wave: the last lane reads codes 252 .. 267

__device__ __forceinline__ uint32_t dna5_code(uint32_t c)
{
    // seqan/basic/alphabet_residue_tabs.h:113-140, as pc_kernels.hip codes the scans' columns
    if (c == 'A' || c == 'a') return 0;
    if (c == 'C' || c == 'c') return 1;
    if (c == 'G' || c == 'g') return 2;
    if (c == 'T' || c == 't' || c == 'U' || c == 'u') return 3;
    return 4;
}

}  // namespace

__global__ __launch_bounds__(256) void kmer_count_kernel(const uint8_t *arena, const int64_t *win_off, const int32_t *win_len,
                                                         int64_t n, int k, uint32_t *counts)
{
    __shared__ __attribute__((aligned(16))) uint8_t strip_all[4][kStrip];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint8_t *strip = strip_all[wv];
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < n; w += nwaves) {
        const int len = win_len[w];
        if (len < k) continue;                                   // (uniform: the whole wave shares the window)
        const uint8_t *base = arena + win_off[w];
        for (int c0 = 0; c0 + k <= len; c0 += kChunk) {
            // bytes [c0, c0 + nb) of the window, nb <= 256 + k - 1 <= 268
            const int nb = (len - c0 < kChunk + k - 1) ? len - c0 : kChunk + k - 1;
            const uint8_t *p = base + c0;
            const int skip = (int)((uintptr_t)p & 3u);
            const uint32_t *q = (const uint32_t *)(p - skip);
            const int ndw = (skip + nb + 3) >> 2;                // <= 68: two dwords per lane at most
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int i = lane + 64 * pass;
                if (i < ndw) {
                    const uint32_t v = q[i];
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int at = 4 * i + b - skip;         // position in the chunk
                        if (at >= 0 && at < nb) strip[at] = (uint8_t)dna5_code((v >> (8 * b)) & 0xFFu);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // (codes past nb are whatever an earlier chunk left: a k-mer that would use one ends outside the window)
            const uint32_t *sw = (const uint32_t *)(strip + 4 * lane);
            uint32_t word = 0, bad = 0;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const uint32_t cw = sw[d];                       // four codes, the first in the lowest byte
                const uint32_t lo = cw & 0x03030303u, hi = (cw >> 2) & 0x01010101u;
                word = (word << 8) | (((lo << 6) | (lo >> 4) | (lo >> 14) | (lo >> 24)) & 0xFFu);
                bad |= ((hi | (hi >> 7) | (hi >> 14) | (hi >> 21)) & 0xFu) << (4 * d);
            }
            const uint32_t kbits = (1u << k) - 1u;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int s = 4 * lane + t;                      // start in the chunk
                if (c0 + s + k <= len && ((bad >> t) & kbits) == 0) {
                    const uint32_t code = (word << (2 * t)) >> (32 - 2 * k);
                    (void)__hip_atomic_fetch_add(counts + code, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            // the next chunk's staging must not overtake this chunk's reads
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

__global__ __launch_bounds__(256) void kmer_select_kernel(const uint32_t *counts, int64_t entries, uint32_t min_count, int32_t *codes,
                                                          uint32_t *cnt, int64_t cap, unsigned long long *found)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // whole waves stay in the loop (entries is a multiple of 256, so is the stride): the ballot is wave-wide
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < entries; c += stride) {
        const uint32_t v = counts[c];
        const bool take = v >= min_count;
        const unsigned long long votes = __ballot(take);
        if (votes == 0) continue;
        const int leader = __ffsll((long long)votes) - 1;
        unsigned long long first = 0;
        if (lane == leader) first = atomicAdd(found, (unsigned long long)__popcll(votes));
        const uint32_t flo = __shfl((int)(uint32_t)first, leader), fhi = __shfl((int)(uint32_t)(first >> 32), leader);
        first = ((unsigned long long)fhi << 32) | flo;
        if (take) {
            const unsigned long long slot = first + (unsigned long long)__popcll(votes & ((1ull << lane) - 1ull));
            if (slot < (unsigned long long)cap) { codes[slot] = (int32_t)c; cnt[slot] = v; }
        }
    }
}

// insert_code_kernel: barcode discovery ("Barcodes").  The scan has aligned one found sequence (the
// anchor) against every end window; a window whose record passes the rule below is ANCHORED, and the L bases right behind
// the anchor (start windows) or before it (end windows) are its insert, returned as one 2-bit code per window -- the
// census's code, first base in the highest bits.  One thread per window, grid-stride: a 32-byte record and at most 32
// byte loads, every one inside the window; latency-bound, nothing to stage.  All products and indices are 64-bit.
__global__ __launch_bounds__(256) void insert_code_kernel(const uint8_t *arena, const int64_t *win_off, const int32_t *win_len,
                                                          const int32_t *records, int64_t n, int anchor_len, int side, int min_identity,
                                                          int L, int64_t *codes)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n; w += stride) {
        const int32_t *rec = records + 8 * w;
        const int64_t read_start = rec[0], read_end = rec[1], ad_start = rec[2], ad_end = rec[3], matches = rec[5], full_len = rec[7];
        int64_t code = -1;
        const bool anchored = read_start >= 0 && full_len > 0 && 100 * matches >= (int64_t)min_identity * full_len &&
                              (side == 0 ? ad_end == (int64_t)anchor_len - 1 : ad_start == 0);
        const int64_t col = side == 0 ? read_end + 1 : read_start - L;
        if (anchored && col >= 0 && col + L <= (int64_t)win_len[w]) {
            const uint8_t *p = arena + win_off[w] + col;
            uint64_t v = 0;
            uint32_t bad = 0;
            for (int i = 0; i < L; ++i) {
                const uint32_t c = dna5_code(p[i]);
                bad |= c;
                v = (v << 2) | (c & 3u);
            }
            if (!(bad & 4u)) code = (int64_t)v;
        }
        codes[w] = code;
    }
}

int launch_anchor_inserts(const uint8_t *arena, const int64_t *win_off, const int32_t *win_len, const int32_t *records, int64_t n,
                          int anchor_len, int side, int min_identity, int insert_len, int64_t *codes, void *stream)
{
    if (n <= 0) return 0;
    const int64_t want = (n + 255) / 256;
    const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
    hipLaunchKernelGGL(insert_code_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, arena, win_off, win_len, records, n, anchor_len,
                       side, min_identity, insert_len, codes);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_kmer_count(const uint8_t *arena, const int64_t *win_off, const int32_t *win_len, int64_t n, int k, uint32_t *counts, void *stream)
{
    if (n <= 0) return 0;
    // four windows per block and pass; enough blocks to fill the chip several times over, the rest by the stride
    const int64_t want = (n + 3) / 4;
    const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
    hipLaunchKernelGGL(kmer_count_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, arena, win_off, win_len, n, k, counts);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_kmer_select(const uint32_t *counts, int k, uint32_t min_count, int32_t *codes, uint32_t *cnt, int64_t cap,
                       unsigned long long *found, void *stream)
{
    const int64_t entries = (int64_t)1 << (2 * k);               // k >= 4: a multiple of 256
    const int64_t want = entries / 256;
    const unsigned grid = (unsigned)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(kmer_select_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, counts, entries, min_count, codes, cnt, cap, found);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace pck
