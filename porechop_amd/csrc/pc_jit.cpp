// pc_jit.cpp -- run-time specialisation of the score-only scan kernel for one adapter pair.
//
// hiprtc is loaded with dlopen (no link-time dependency); if it is missing, or a compile fails,
// pcj::get() returns null and the caller keeps using the ahead-of-time generic kernels -- still
// the GPU, only 9 instead of 5 (fp16) / 6 (int16) packed ops per cell pair.  PC_DISABLE_JIT=1
// forces that path.
#include "pc_jit.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "pc_bounds.h"
#include "pc_letters.h"
#include "pc_jit_source.h"

namespace pcj {

namespace {

typedef struct _hiprtcProgram *hiprtcProgram;
typedef int hiprtcResult;
struct Rtc {
    void *lib = nullptr;
    hiprtcResult (*CreateProgram)(hiprtcProgram *, const char *, const char *, int, const char *const *, const char *const *) = nullptr;
    hiprtcResult (*CompileProgram)(hiprtcProgram, int, const char *const *) = nullptr;
    hiprtcResult (*GetProgramLogSize)(hiprtcProgram, size_t *) = nullptr;
    hiprtcResult (*GetProgramLog)(hiprtcProgram, char *) = nullptr;
    hiprtcResult (*GetCodeSize)(hiprtcProgram, size_t *) = nullptr;
    hiprtcResult (*GetCode)(hiprtcProgram, char *) = nullptr;
    hiprtcResult (*DestroyProgram)(hiprtcProgram *) = nullptr;
    bool ok = false;
};

Rtc &rtc()
{
    static Rtc r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *names[] = {"libhiprtc.so.7", "libhiprtc.so", "libhiprtc.so.6"};
        for (const char *n : names) { r.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL); if (r.lib) break; }
        if (!r.lib) return;
#define PC_SYM(field, sym) *(void **)(&r.field) = dlsym(r.lib, sym); if (!r.field) return;
        PC_SYM(CreateProgram, "hiprtcCreateProgram")
        PC_SYM(CompileProgram, "hiprtcCompileProgram")
        PC_SYM(GetProgramLogSize, "hiprtcGetProgramLogSize")
        PC_SYM(GetProgramLog, "hiprtcGetProgramLog")
        PC_SYM(GetCodeSize, "hiprtcGetCodeSize")
        PC_SYM(GetCode, "hiprtcGetCode")
        PC_SYM(DestroyProgram, "hiprtcDestroyProgram")
#undef PC_SYM
        r.ok = true;
    });
    return r;
}

int dna5(unsigned char c)
{
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return 4;
    }
}

// IEEE half bit pattern of a small integer (|v| <= 2048 is exact)
uint32_t half_bits(int v)
{
    if (v == 0) return 0;
    const uint32_t sign = v < 0 ? 0x8000u : 0u;
    uint32_t a = (uint32_t)(v < 0 ? -v : v);
    int e = 0;
    while ((a >> (e + 1)) != 0) ++e;                 // floor(log2(a)), <= 11
    const uint32_t mant = e <= 10 ? ((a << (10 - e)) & 0x3FFu) : ((a >> (e - 10)) & 0x3FFu);
    return sign | ((uint32_t)(e + 15) << 10) | mant;
}

// One adapter pair + scheme: its specialised kernel goes through
//   ABSENT (work seen so far below the threshold) -> COMPILING (hiprtc, possibly on a worker
//   thread) -> READY (module loaded, table uploaded) | FAILED (never retried)
struct Entry {
    enum State { ABSENT, COMPILING, READY, FAILED } state = ABSENT;
    double seen = 0;                 // cells scanned with the generic kernel so far
    bool disk_checked = false;       // the kernel caches on disk were looked at (once per entry)
    bool from_disk = false;
    Spec *spec = nullptr;
    // product of the compile step (no HIP calls in it: it may run on a worker thread)
    std::vector<char> code;
    std::vector<uint32_t> table;
    std::string log;
    bool compiled_ok = false;
    std::atomic<bool> compile_done{false};
    std::thread worker;
    int R = 0, K = 0, m_lo = 0, m_hi = 0, waves = 2, r0 = 0;
    bool f16 = false, top = false;
    long kren = 0;
};

std::mutex g_mu;                               // the cache
std::mutex g_compile_mu;                       // one hiprtc compile at a time
std::map<std::string, Entry *> g_cache;
std::atomic<int> g_async{0};
std::atomic<bool> g_cancel{false};             // set at shutdown: queued compiles are dropped

struct Recipe {                                // everything the compile step needs, by value
    std::string ad_lo, ad_hi;
    int match, mismatch, gap_open, gap_extend;
    int R, m_lo, m_hi, eps, waves;
    bool f16;
    long kren, cen;
    bool row_skip = false;                     // the variant whose fast path skips the rows below r0 (a kernel of its own per pair)
    bool wildcards = false;                    // the adapters' letters are IUPAC sets (pc_letters.h): same source, other letter pairs and table
};

// Everything about a kernel that follows from its recipe without compiling anything: the hiprtc options (they
// ARE the kernel's identity: the source is one constant string), the distinct letter pairs, the register plan.
struct Derived {
    std::vector<std::string> opts;
    std::vector<int> combos;
    int K = 0, waves = 2, r0 = 0;
    bool top = false;                          // the row-skipping variant with the shorter adapter top-aligned (pc_bounds.h row_skip_plan_top)
};

constexpr int kPadLetter = 32, kLetters = 33;    // a letter is a 5-bit set, or the padding row

// the row rule of the top-aligned layout simulates (pcb::row_skip_r0_top: a quarter of a second): once per recipe and process
int top_rule_r0(const Recipe &rc)
{
    static std::mutex mu;
    static std::map<std::string, int> memo;
    char buf[96];
    snprintf(buf, sizeof buf, "|%d,%d,%d,%d|%d", rc.match, rc.mismatch, rc.gap_open, rc.gap_extend, rc.wildcards ? 1 : 0);
    const std::string key = rc.ad_lo + "|" + rc.ad_hi + buf;
    std::lock_guard<std::mutex> lk(mu);
    auto it = memo.find(key);
    if (it != memo.end()) return it->second;
    unsigned char sl[pcb::MAX_ADAPTER], sh[pcb::MAX_ADAPTER];
    for (int i = 0; i < rc.m_lo; ++i) sl[i] = (unsigned char)pcl::letter_set((uint8_t)rc.ad_lo[i], rc.wildcards);
    for (int i = 0; i < rc.m_hi; ++i) sh[i] = (unsigned char)pcl::letter_set((uint8_t)rc.ad_hi[i], rc.wildcards);
    const int r0 = pcb::row_skip_r0_top(rc.match, rc.mismatch, rc.gap_open, rc.gap_extend, rc.R, rc.m_lo, rc.m_hi, sl, sh);
    memo[key] = r0;
    return r0;
}

Derived derive(const Recipe &rc)
{
    Derived d;
    const int R = rc.R;
    const char *chk = getenv("PC_JIT_CHECK_RANGE");
    const bool check_range = chk && *chk && *chk != '0';
    // the distinct letter pairs of the rows, numbered in row order (pc_letters.h: one code without wildcards, so rows are told
    // apart exactly as their Dna5 codes were and the options of such adapters are what they have always been)
    auto number_rows = [&](const std::vector<int> &lo, const std::vector<int> &hi, std::vector<int> &combo_of_row) {
        d.combos.clear();
        combo_of_row.assign(R, 0);
        for (int row = 0; row < R; ++row) {
            const int c = lo[row] * kLetters + hi[row];
            int k = -1;
            for (size_t i = 0; i < d.combos.size(); ++i) if (d.combos[i] == c) k = (int)i;
            if (k < 0) { k = (int)d.combos.size(); d.combos.push_back(c); }
            combo_of_row[row] = k;
        }
    };
    auto options = [&](const std::vector<int> &combo_of_row, int K, int waves) {
        std::string init;
        for (int row = 0; row < R; ++row) { init += std::to_string(combo_of_row[row]); if (row + 1 < R) init += ","; }
        d.opts = {"--offload-arch=gfx950", "-O3", "-std=c++17",
                  "-DPC_R=" + std::to_string(R), "-DPC_K=" + std::to_string(K), "-DPC_COMBO_INIT=" + init,
                  std::string("-DPC_F16=") + (rc.f16 ? "1" : "0"), "-DPC_EPS=" + std::to_string(rc.eps),
                  "-DPC_OE=(" + std::to_string(rc.gap_open + rc.eps) + ")", "-DPC_CEN=(" + std::to_string(rc.cen) + ")",
                  "-DPC_KREN=" + std::to_string(rc.kren),
                  std::string("-DPC_WAVES=") + (getenv("PC_JIT_WAVES") ? getenv("PC_JIT_WAVES") : std::to_string(waves)),
                  std::string("-DPC_CHECK_RANGE=") + (check_range ? "1" : "0"),
                  std::string("-DPC_DUAL=") + (rc.ad_lo != rc.ad_hi ? "1" : "0")};
    };
    // PC_JIT_R0 overrides a rule's row (measurements): one row for every pair ("20") or a row per pair ("28|22:20,33|30:22"),
    // pcb::row_skip_r0_override; a malformed text is ignored, a row the layout cannot use means no variant (R)
    auto overridden = [&](int rule_r0, auto usable) {
        const char *e = getenv("PC_JIT_R0");
        if (!e) return rule_r0;
        bool malformed = false;
        const int v = pcb::row_skip_r0_override(e, rc.m_lo, rc.m_hi, rule_r0, &malformed);
        if (malformed) {
            static std::atomic<bool> said{false};
            if (!said.exchange(true)) fprintf(stderr, "porechop_amd: PC_JIT_R0=%s is not a row or a list of LEN|LEN:ROW entries; ignored\n", e);
            return rule_r0;
        }
        return v == rule_r0 ? rule_r0 : (usable(v) ? v : R);
    };
    // the kernel's LDS (tables, three look-up tables, 512 bytes per lower row) times the twelve workgroups of a CU at three
    // waves per SIMD must fit its 160 KiB, or the variant would run at a lower occupancy than the plain kernel: then none
    auto lds_fits = [&](int K, int r0) { return 12L * (100L * K + 1536 + 512L * (R - r0)) <= 160L * 1024; };

    // ---- The row-skipping variant of a pair of DIFFERENT lengths: the shorter adapter top-aligned (pc_bounds.h row_skip_plan_top),
    // register row = adapter row in both halves, the padding letter below the shorter one.  No padding sits above the row the
    // fast path tests, which lets that row sit lower.  The rows are numbered in row order, so the letter pairs of the rows
    // above r0 are the first ones: the fast path fetches only the first PC_KUP terms of a column (the lower part and the
    // one-column path read the full row), and it is the fast path's registers -- T, U and four sets of PC_KUP terms -- that
    // decide the waves.  Three-wave kernels only, as below.  PC_SKIP_LAYOUT=bottom compiles the bottom-aligned variant
    // instead (A/B runs: the options differ, so the caches keep both).  A pair whose top-aligned variant has no row by the
    // rule, or no room, gets the bottom-aligned one if that has.  Not so under PC_JIT_R0: a row asked for in its place that
    // this layout cannot use or has no room for means NO variant (the plain kernel runs), never the other layout at that
    // row -- a measurement must not be of a layout it did not ask for.
    // (No room whatever the row -- K_up >= 4, so 2R + 16 > 120 -- is found before the rule's simulation is paid for.)
    const char *layout = getenv("PC_SKIP_LAYOUT");
    bool no_variant = false;
    if (rc.row_skip && rc.f16 && !check_range && rc.m_lo != rc.m_hi && 2 * R + 16 <= 120 && !(layout && !strcmp(layout, "bottom"))) {
        std::vector<int> lo(R, kPadLetter), hi(R, kPadLetter), combo_of_row;
        for (int i = 0; i < rc.m_lo; ++i) lo[i] = (int)pcl::letter_set((uint8_t)rc.ad_lo[i], rc.wildcards);
        for (int i = 0; i < rc.m_hi; ++i) hi[i] = (int)pcl::letter_set((uint8_t)rc.ad_hi[i], rc.wildcards);
        number_rows(lo, hi, combo_of_row);
        const int K = ((int)d.combos.size() + 3) / 4 * 4;
        const int m_min = std::min(rc.m_lo, rc.m_hi);
        const int rule_r0 = top_rule_r0(rc);
        const int r0 = overridden(rule_r0, [&](int v) { return v >= 2 && !(v & 1) && v < m_min; });
        if (const char *e = getenv("PC_JIT_R0")) {           // a row asked for for this pair: this layout at that row, or nothing
            bool malformed = false;
            no_variant = pcb::row_skip_r0_override(e, rc.m_lo, rc.m_hi, -1, &malformed) != -1;
        }
        if (r0 < R) {
            int k_up = 0;
            for (int row = 0; row < r0; ++row) k_up = std::max(k_up, combo_of_row[row] + 1);
            k_up = (k_up + 3) / 4 * 4;
            if (2 * R + 4 * k_up <= 120 && lds_fits(K, r0)) {
                d.K = K; d.waves = 3; d.r0 = r0; d.top = true;
                options(combo_of_row, K, 3);
                d.opts.push_back("-DPC_R0=" + std::to_string(r0));
                d.opts.push_back("-DPC_TOP=1");
                d.opts.push_back("-DPC_MLO=" + std::to_string(rc.m_lo));
                d.opts.push_back("-DPC_MHI=" + std::to_string(rc.m_hi));
                d.opts.push_back("-DPC_KUP=" + std::to_string(k_up));
                return d;
            }
        }
    }

    // letters per register row of each half (bottom-aligned), kPadLetter = padding row
    std::vector<int> lo(R, kPadLetter), hi(R, kPadLetter), combo_of_row;
    for (int i = 0; i < rc.m_lo; ++i) lo[R - rc.m_lo + i] = (int)pcl::letter_set((uint8_t)rc.ad_lo[i], rc.wildcards);
    for (int i = 0; i < rc.m_hi; ++i) hi[R - rc.m_hi + i] = (int)pcl::letter_set((uint8_t)rc.ad_hi[i], rc.wildcards);
    number_rows(lo, hi, combo_of_row);
    const int K = ((int)d.combos.size() + 3) / 4 * 4;
    // Register budget: T, U and four sets of substitution terms (two columns in flight, two being
    // fetched) = 2R + 4K, plus ~50 of bookkeeping.  Up to 120 the column loop fits 168 VGPRs -- three waves
    // per SIMD, the few values the allocator then spills are touched only outside the loop (measured: -5 %
    // on the 28+22-base pair, -4 % on 33+30; a 39+34-base pair, 142, spills inside the loop and loses 10 %).
    // Up to 140: 256 VGPRs, two waves.  Longer adapters (full barcode sequences, 63-111 bases) get the whole
    // register file of a SIMD -- one wave, the rows beyond 256 VGPRs parked in AGPRs -- which is still
    // several times faster than the generic kernel's column in LDS.
    const int waves = (2 * R + 4 * K <= 120) ? 3 : (2 * R + 4 * K <= 140) ? 2 : 1;
    d.K = K; d.waves = waves;
    // the row its row-skipping fast path tests (pc_bounds.h): packed fp16 only, and not in the range-recording build, which
    // takes the one-column path throughout.  Three-wave kernels only: the longer pairs' kernels (two waves, or one with rows
    // parked in AGPRs) have no room for the lower part beside their rows, and their few workgroups per CU would pay for the
    // lower rows' LDS with occupancy.  PC_JIT_R0 overrides the rule (measurements; an unusable row means none)
    const bool may_skip = rc.row_skip && rc.f16 && !check_range && waves == 3 && !no_variant;
    d.r0 = may_skip ? pcb::row_skip_r0(rc.match, rc.mismatch, rc.gap_open, rc.gap_extend, R, rc.m_lo, rc.m_hi) : R;
    if (may_skip) {
        const int pad = R - std::min(rc.m_lo, rc.m_hi);
        d.r0 = overridden(d.r0, [&](int v) { return v >= 2 && !(v & 1) && v < R && v > pad; });
    }
    if (d.r0 < R && !lds_fits(K, d.r0)) d.r0 = R;
    options(combo_of_row, K, waves);
    if (d.r0 < R) d.opts.push_back("-DPC_R0=" + std::to_string(d.r0));        // (the plain kernel's options are what they were)
    return d;
}

// S table: [code of the low stream's base * 5 + code of the high stream's base][K letter pairs] of packed
// (sub_lo - open + eps) | (sub_hi - open + eps) << 16
std::vector<uint32_t> substitution_table(const Recipe &rc, const Derived &d)
{
    std::vector<uint32_t> table((size_t)25 * d.K, 0);
    auto term = [&](int letter, int code) -> int {
        const int sub = letter == kPadLetter ? 0 : (pcl::matches((unsigned)letter, code) ? rc.match : rc.mismatch);
        return sub - rc.gap_open + rc.eps;
    };
    for (int cl = 0; cl < 5; ++cl)
        for (int ch = 0; ch < 5; ++ch)
            for (size_t k = 0; k < d.combos.size(); ++k) {
                const int l = term(d.combos[k] / kLetters, cl), h = term(d.combos[k] % kLetters, ch);
                // the table terms are values the kernel adds in its lane type: they must be exact there too
                // (spec_plan's gate bounds match, mismatch and open for the fp16 variant; asserted here, where they are formed)
                const int lim = rc.f16 ? pcb::kF16Limit : 32000;
                if (l > lim || l < -lim || h > lim || h < -lim) return std::vector<uint32_t>();
                table[(size_t)(cl * 5 + ch) * d.K + k] = rc.f16 ? (half_bits(l) | (half_bits(h) << 16))
                                                                : (((uint32_t)l & 0xFFFFu) | ((uint32_t)h << 16));
            }
    return table;
}

// ---- kernel cache on disk ------------------------------------------------------------------------------
// A specialised kernel is a pure function of (kSpecSource, hiprtc options).  Its code object is kept in a file
// named by a 128-bit hash of both; the file repeats the options, and a load checks them and the source's own
// hash, so a collision or a stale file can only cause a recompile.  Two directories are consulted:
//   <directory of this library>/kernel_cache   read-only: filled at build time for the static panel
//                                              (pc_jit_precompile; `make kernels`, __graft_entry__.build())
//   PC_JIT_CACHE_DIR, else $XDG_CACHE_HOME/porechop_amd, else $HOME/.cache/porechop_amd
//                                              read-write: what this machine compiled at run time
// PC_JIT_CACHE_DIR=off (or 0) disables the second one.
uint64_t fnv64(const void *p, size_t n, uint64_t h)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}

const char kCacheMagic[] = "PCJK3\n";

// The toolchain a cached code object belongs to: the HIP / clang versions THIS LIBRARY was compiled with (hipcc and
// hiprtc of one ROCm install share their compiler; the library is built in-tree by that install).  Part of the file
// name's hash and of the header a load checks, so code objects in ~/.cache/porechop_amd or in a copied kernel_cache/
// do not survive a toolchain upgrade: they simply stop being found and are recompiled.
#define PC_STR2(x) #x
#define PC_STR(x) PC_STR2(x)
const char kToolchainTag[] = "toolchain=hip-" PC_STR(HIP_VERSION_MAJOR) "." PC_STR(HIP_VERSION_MINOR) "." PC_STR(HIP_VERSION_PATCH)
                             "/clang-" __clang_version__;

std::string joined(const std::vector<std::string> &opts)
{
    std::string s;
    for (const std::string &o : opts) { s += o; s += ' '; }
    s += kToolchainTag;
    return s;
}

uint64_t source_hash()
{
    static const uint64_t h = fnv64(kSpecSource, strlen(kSpecSource), 0xcbf29ce484222325ull);
    return h;
}

std::string cache_file_name(const std::vector<std::string> &opts)
{
    const std::string o = joined(opts);
    const uint64_t h1 = fnv64(o.data(), o.size(), source_hash());
    const uint64_t h2 = fnv64(o.data(), o.size(), source_hash() * 0x9E3779B97F4A7C15ull + 0x632be59bd9b4e019ull);
    char buf[64];
    snprintf(buf, sizeof buf, "%016llx%016llx.pcjk", (unsigned long long)h1, (unsigned long long)h2);
    return buf;
}

std::string library_dir()
{
    Dl_info info;
    if (dladdr((void *)&fnv64, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        const size_t k = p.rfind('/');
        return k == std::string::npos ? std::string(".") : p.substr(0, k);
    }
    return ".";
}

std::string intree_cache_dir() { static const std::string d = library_dir() + "/kernel_cache"; return d; }

std::string user_cache_dir()
{
    const char *e = getenv("PC_JIT_CACHE_DIR");
    if (e) {
        if (!*e || !strcmp(e, "0") || !strcmp(e, "off")) return "";
        return e;
    }
    const char *x = getenv("XDG_CACHE_HOME");
    if (x && *x) return std::string(x) + "/porechop_amd";
    const char *h = getenv("HOME");
    if (h && *h) return std::string(h) + "/.cache/porechop_amd";
    return "";
}

void make_dirs(const std::string &dir)
{
    for (size_t k = 1; k <= dir.size(); ++k)
        if (k == dir.size() || dir[k] == '/') (void)mkdir(dir.substr(0, k).c_str(), 0755);
}

bool cache_read(const std::string &dir, const std::vector<std::string> &opts, std::vector<char> &code)
{
    if (dir.empty()) return false;
    const std::string path = dir + "/" + cache_file_name(opts);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    bool ok = false;
    const std::string want = joined(opts);
    char magic[sizeof kCacheMagic] = {0};
    uint64_t src = 0, olen = 0, clen = 0;
    std::string got;
    if (fread(magic, 1, sizeof kCacheMagic - 1, f) == sizeof kCacheMagic - 1 && !strcmp(magic, kCacheMagic) &&
        fread(&src, 8, 1, f) == 1 && src == source_hash() && fread(&olen, 8, 1, f) == 1 && olen == want.size()) {
        got.resize(olen);
        if (fread(&got[0], 1, olen, f) == olen && got == want && fread(&clen, 8, 1, f) == 1 && clen > 0 && clen < (1ull << 28)) {
            code.resize(clen);
            uint64_t sum = 0;
            ok = fread(code.data(), 1, clen, f) == clen && fread(&sum, 8, 1, f) == 1 &&
                 sum == fnv64(code.data(), clen, 0xcbf29ce484222325ull);
        }
    }
    fclose(f);
    if (!ok) code.clear();
    return ok;
}

bool cache_write(const std::string &dir, const std::vector<std::string> &opts, const std::vector<char> &code)
{
    if (dir.empty() || code.empty()) return false;
    make_dirs(dir);
    const std::string path = dir + "/" + cache_file_name(opts);
    char tmp[64];
    snprintf(tmp, sizeof tmp, ".tmp%ld_%p", (long)getpid(), (const void *)&code);
    const std::string tpath = path + tmp;
    FILE *f = fopen(tpath.c_str(), "wb");
    if (!f) return false;
    const std::string o = joined(opts);
    const uint64_t src = source_hash(), olen = o.size(), clen = code.size(), sum = fnv64(code.data(), code.size(), 0xcbf29ce484222325ull);
    bool ok = fwrite(kCacheMagic, 1, sizeof kCacheMagic - 1, f) == sizeof kCacheMagic - 1 && fwrite(&src, 8, 1, f) == 1 &&
              fwrite(&olen, 8, 1, f) == 1 && fwrite(o.data(), 1, olen, f) == olen && fwrite(&clen, 8, 1, f) == 1 &&
              fwrite(code.data(), 1, clen, f) == clen && fwrite(&sum, 8, 1, f) == 1;
    ok = (fclose(f) == 0) && ok;
    if (ok) ok = rename(tpath.c_str(), path.c_str()) == 0;      // atomic: readers see a whole file or none
    if (!ok) (void)unlink(tpath.c_str());
    return ok;
}

std::atomic<long> g_n_compiled{0}, g_n_disk{0};

// hiprtc compile of one kernel.  No HIP runtime calls (hiprtc needs no device).
bool hiprtc_compile(const std::vector<std::string> &opts, std::vector<char> &code, std::string &log)
{
    Rtc &r = rtc();                      // first use loads libhiprtc (hundreds of ms)
    if (!r.ok) { log = "hiprtc not available"; return false; }
    std::vector<const char *> o;
    for (const std::string &s : opts) o.push_back(s.c_str());
    hiprtcProgram prog = nullptr;
    bool ok = false;
    if (r.CreateProgram(&prog, kSpecSource, "pc_spec_score.hip", 0, nullptr, nullptr) == 0) {
        const hiprtcResult rcode = r.CompileProgram(prog, (int)o.size(), o.data());
        if (rcode != 0) {
            size_t n = 0;
            r.GetProgramLogSize(prog, &n);
            log.assign(n + 1, '\0');
            if (n) r.GetProgramLog(prog, &log[0]);
        } else {
            size_t csz = 0;
            r.GetCodeSize(prog, &csz);
            code.resize(csz);
            r.GetCode(prog, code.data());
            ok = csz > 0;
        }
        r.DestroyProgram(&prog);
    } else {
        log = "hiprtcCreateProgram failed";
    }
    return ok;
}

void fill_entry(Entry *e, const Recipe &rc, const Derived &d)
{
    e->R = rc.R; e->K = d.K; e->m_lo = rc.m_lo; e->m_hi = rc.m_hi; e->f16 = rc.f16; e->waves = d.waves; e->r0 = d.r0; e->top = d.top; e->kren = rc.kren;
    e->table = substitution_table(rc, d);           // empty: a table term outside the lane type's exact range (never expected)
}

// The kernel from one of the caches on disk, if it is there.  No HIP runtime calls.
bool load_entry_from_disk(Entry *e, const Recipe &rc)
{
    const Derived d = derive(rc);
    if (!cache_read(intree_cache_dir(), d.opts, e->code) && !cache_read(user_cache_dir(), d.opts, e->code)) return false;
    fill_entry(e, rc, d);
    if (e->table.empty()) { e->code.clear(); return false; }
    e->compiled_ok = true;
    e->from_disk = true;
    g_n_disk.fetch_add(1);
    return true;
}

// hiprtc compile + substitution table (+ a copy of the code object in the user's cache directory).
// No HIP runtime calls: it may run on a worker thread.
void compile_entry(Entry *e, const Recipe rc)
{
    std::lock_guard<std::mutex> one(g_compile_mu);
    if (g_cancel.load()) { e->log = "cancelled"; e->compile_done.store(true, std::memory_order_release); return; }
    const Derived d = derive(rc);
    fill_entry(e, rc, d);
    e->compiled_ok = !e->table.empty() && hiprtc_compile(d.opts, e->code, e->log);
    if (e->table.empty()) e->log = "a substitution-table term lies outside the lane type's exact range";
    if (e->compiled_ok) {
        g_n_compiled.fetch_add(1);
        (void)cache_write(user_cache_dir(), d.opts, e->code);
    }
    e->compile_done.store(true, std::memory_order_release);
}

// Module load + table upload on the caller's thread (the one that owns the device context).
void finalize_entry(Entry *e, bool verbose)
{
    if (e->worker.joinable()) e->worker.join();
    e->state = Entry::FAILED;
    if (!e->compiled_ok) {
        static bool told = false;
        if (!told || e->log != "hiprtc not available")
            fprintf(stderr, "porechop_amd: no specialised kernel (%s), using the generic scan kernels\n", e->log.c_str());
        told = true;
        return;
    }
    Spec *sp = new Spec();
    sp->R = e->R; sp->K = e->K; sp->m_lo = e->m_lo; sp->m_hi = e->m_hi; sp->f16 = e->f16; sp->waves = e->waves; sp->r0 = e->r0; sp->top = e->top;
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    if (hipModuleLoadData(&mod, e->code.data()) != hipSuccess || hipModuleGetFunction(&fn, mod, "pc_spec_score") != hipSuccess) {
        fprintf(stderr, "porechop_amd: loading the specialised kernel failed, using the generic kernels\n");
        delete sp;
        return;
    }
    sp->module = mod; sp->function = fn;
    // resident workgroups (= waves) per CU as the runtime sees them -- registers AND LDS -- for the launch
    // planner's balanced heads (pc_api.cpp plan_score_launches)
    int nb = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 64, 0) == hipSuccess && nb > 0) sp->blocks_per_cu = nb;
    else sp->blocks_per_cu = 4 * e->waves;
    void *d = nullptr;
    if (hipMalloc(&d, e->table.size() * 4) != hipSuccess ||
        hipMemcpy(d, e->table.data(), e->table.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        delete sp;
        return;
    }
    sp->d_table = d;
    if (verbose) fprintf(stderr, "porechop_amd: specialised kernel R=%d K=%d f16=%d kren=%ld waves/CU=%d (%s)\n", e->R, e->K, e->f16 ? 1 : 0, e->kren, sp->blocks_per_cu, e->from_disk ? "from the kernel cache on disk" : "compiled now");
    e->code.clear(); e->code.shrink_to_fit();
    e->spec = sp;
    e->state = Entry::READY;
}

}  // namespace

bool disabled()
{
    const char *e = getenv("PC_DISABLE_JIT");
    return e && *e && *e != '0';
}

void set_async(int on) { g_async.store(on ? 1 : 0); }

void wait_idle(bool cancel_queued)
{
    // a worker must not be inside hiprtc when the process image is torn down: callers with
    // asynchronous specialisation on call this before exiting (the Python binding registers it with
    // atexit).  Compiles that have not started yet are dropped; the one in flight is waited for.
    if (cancel_queued) g_cancel.store(true);
    std::vector<Entry *> es;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        for (auto &kv : g_cache) es.push_back(kv.second);
    }
    for (Entry *e : es) if (e->worker.joinable()) e->worker.join();
}

namespace {
// a worker thread must not be inside hiprtc while the process image is torn down, whoever loaded the library
struct JoinAtExit { ~JoinAtExit() { wait_idle(true); } } g_join_at_exit;
}  // namespace

Spec *get(int device, const std::string &ad_lo, const std::string &ad_hi, int match, int mismatch, int gap_open,
          int gap_extend, double cells, bool int16_only, bool row_skip, bool wildcards)
{
    if (disabled()) return nullptr;
    const int m_lo = (int)ad_lo.size(), m_hi = (int)ad_hi.size();
    const int R = m_lo > m_hi ? m_lo : m_hi;
    static const bool verbose = [] { const char *v = getenv("PC_JIT_VERBOSE"); return v && *v && *v != '0'; }();
    if (R < 2 || R > pcb::MAX_ADAPTER) {
        if (verbose) fprintf(stderr, "porechop_amd: no specialised kernel for %d rows\n", R);
        return nullptr;
    }
    // Drifting coordinates (pc_jit_source.h): a value X of row rho, jj columns after the last
    // renormalisation, is held as X + (rho + jj [+1]) * eps - C.  True values lie in
    // [low, high]; C puts `low` at -lim and the renormalisation period KREN keeps the top below
    // +lim, lim = what the lane type holds exactly (fp16: integers up to 2048).  Packed-fp16
    // variant (5 ops per cell pair, v_pk_maximum3_f16) when that leaves a useful period, otherwise
    // packed-int16 (6 ops).  PC_JIT_INT16=1 forces the latter.
    const int eps = -gap_extend;
    const char *force_int = getenv("PC_JIT_INT16");
    const pcb::SpecPlan plan = pcb::spec_plan(match, mismatch, gap_open, gap_extend, R, int16_only || (force_int && *force_int && *force_int != '0'));
    const bool f16 = plan.f16;
    const long kren = plan.kren;
    if (!plan.ok) {
        if (verbose) fprintf(stderr, "porechop_amd: no specialised kernel: scores too large for drifting coordinates\n");
        return nullptr;
    }
    const long cen = plan.cen;
    char keybuf[96];
    if (row_skip) {
        // the row-skipping variant exists for packed fp16 and where the rule finds a row (a function of the recipe alone)
        const Recipe probe{ad_lo, ad_hi, match, mismatch, gap_open, gap_extend, R, m_lo, m_hi, eps, 2, f16, kren, plan.cen, true, wildcards};
        if (!f16 || derive(probe).r0 >= R) return nullptr;
    }
    if (wildcards) {
        // degenerate letters make more distinct letter pairs (K) and so more registers: beyond the largest plan Dna5 letters
        // can ask for (128 rows, 36 pairs) there is no room, and the generic kernel runs
        const Recipe probe{ad_lo, ad_hi, match, mismatch, gap_open, gap_extend, R, m_lo, m_hi, eps, 2, f16, kren, plan.cen, false, true};
        // (and K itself stays within the 36 pairs Dna5 letters can make: the one-wave plan parks rows, not table terms)
        const int K = derive(probe).K;
        if (K > 36 || 2 * R + 4 * K > 2 * pcb::MAX_ADAPTER + 4 * 36) {
            if (verbose) fprintf(stderr, "porechop_amd: no specialised kernel: too many distinct letter pairs for the register plan\n");
            return nullptr;
        }
    }
    // (the mode is part of the key: ACGN has the same code object in both modes and another table)
    snprintf(keybuf, sizeof keybuf, "|%d|%d,%d,%d,%d|%d%s%s", device, match, mismatch, gap_open, gap_extend, f16 ? 1 : 0, row_skip ? "|skip" : "",
             wildcards ? "|wild" : "");
    const std::string key = ad_lo + "|" + ad_hi + keybuf;
    std::lock_guard<std::mutex> lk(g_mu);
    Entry *&slot = g_cache[key];
    if (!slot) slot = new Entry();
    Entry *e = slot;
    if (e->state == Entry::READY) return e->spec;
    if (e->state == Entry::FAILED) return nullptr;
    if (e->state == Entry::COMPILING) {
        // asynchronous mode: the generic kernel keeps running until the worker is done
        if (!e->compile_done.load(std::memory_order_acquire)) return nullptr;
        finalize_entry(e, verbose);
        return e->spec;
    }
    const Recipe rc{ad_lo, ad_hi, match, mismatch, gap_open, gap_extend, R, m_lo, m_hi, eps, 2, f16, kren, cen, row_skip, wildcards};
    // a kernel that is already on disk (built with the library for the static panel, or compiled by an earlier
    // process on this machine) costs a file read and a module load: use it from the first launch on
    if (!e->disk_checked) {
        e->disk_checked = true;
        if (load_entry_from_disk(e, rc)) {
            e->compile_done.store(true, std::memory_order_release);
            finalize_entry(e, verbose);
            return e->spec;
        }
    }
    // a hiprtc compile costs 0.3-2 s and halves the scan (x6-10 for long adapters): start it once
    // the work seen for this adapter pair, over all launches so far, would have paid for it
    // (PC_JIT_MIN_CELLS overrides the 1e11-cell default)
    static const double min_cells = [] { const char *v = getenv("PC_JIT_MIN_CELLS"); return v ? atof(v) : 1e11; }();
    e->seen += cells;
    if (e->seen < min_cells) return nullptr;
    e->state = Entry::COMPILING;
    // Compile in place only when THIS launch alone is worth the stall; a small launch that merely tipped
    // the pair's running total over the threshold (the mask-and-realign rounds: a millisecond of work)
    // never waits 0.3 s for a compile -- the worker thread builds the kernel, this launch and the next
    // ones use the generic kernel, a later one picks the result up.
    if (g_async.load() || cells < min_cells) {
        e->worker = std::thread(compile_entry, e, rc);
        return nullptr;
    }
    compile_entry(e, rc);
    finalize_entry(e, verbose);
    return e->spec;
}

int precompile(const std::string &ad_lo, const std::string &ad_hi, int match, int mismatch, int gap_open, int gap_extend,
               const std::string &dir, bool row_skip)
{
    const int m_lo = (int)ad_lo.size(), m_hi = (int)ad_hi.size();
    const int R = m_lo > m_hi ? m_lo : m_hi;
    if (R < 2 || R > pcb::MAX_ADAPTER || m_lo < 1 || m_hi < 1) return -1;
    if (pcb::is_linear(gap_open, gap_extend) || !pcb::scores_supported(match, mismatch, gap_open, gap_extend, R)) return -1;
    const char *force_int = getenv("PC_JIT_INT16");
    const pcb::SpecPlan plan = pcb::spec_plan(match, mismatch, gap_open, gap_extend, R, force_int && *force_int && *force_int != '0');
    if (!plan.ok) return -1;
    const Recipe rc{ad_lo, ad_hi, match, mismatch, gap_open, gap_extend, R, m_lo, m_hi, -gap_extend, 2, plan.f16, plan.kren, plan.cen, row_skip};
    const Derived d = derive(rc);
    if (row_skip && d.r0 >= R) return 2;                       // the pair has no row-skipping variant
    const std::string where = dir.empty() ? intree_cache_dir() : dir;
    std::vector<char> code;
    if (cache_read(where, d.opts, code)) return 1;
    std::string log;
    if (!hiprtc_compile(d.opts, code, log)) {
        fprintf(stderr, "porechop_amd: precompile failed: %s\n", log.c_str());
        return -2;
    }
    return cache_write(where, d.opts, code) ? 0 : -3;
}

void stats(long *compiled, long *from_disk)
{
    if (compiled) *compiled = g_n_compiled.load();
    if (from_disk) *from_disk = g_n_disk.load();
}

bool row_skip_args(const Spec *sp, int match, int mismatch, int gap_open, int gap_extend, int32_t floor_lo, int32_t floor_hi, SpecArgs &a)
{
    a.skip_thr2 = 0; a.skip_w = 0;
    if (!sp || !sp->f16 || sp->r0 <= 0 || sp->r0 >= sp->R || floor_lo == INT32_MIN || floor_hi == INT32_MIN) return false;
    // (thresholds and window of the layout the kernel was compiled with)
    const pcb::RowSkip p = sp->top ? pcb::row_skip_plan_top(match, mismatch, gap_open, gap_extend, sp->R, sp->r0, sp->m_lo, sp->m_hi, floor_lo, floor_hi)
                                   : pcb::row_skip_plan(match, mismatch, gap_open, gap_extend, sp->R, sp->r0, sp->m_lo, sp->m_hi, floor_lo, floor_hi);
    if (!p.ok) return false;
    // what M(r0, j) + r0 * eps must exceed: an integer of magnitude <= match * m + R * eps, exact in fp16 by spec_plan's gate
    const int eps = -gap_extend;
    a.skip_thr2 = half_bits(p.theta_lo + sp->r0 * eps - 1) | (half_bits(p.theta_hi + sp->r0 * eps - 1) << 16);
    a.skip_w = p.w_low;
    return true;
}

int launch(const Spec *sp, const SpecArgs &a, int grid, void *stream)
{
    SpecArgs args = a;
    args.s_table = (const uint32_t *)sp->d_table;
    args.m_lo = sp->m_lo; args.m_hi = sp->m_hi;
    args.one2 = 0x00010001u;
    void *params[] = {&args};
    const hipError_t e = hipModuleLaunchKernel((hipFunction_t)sp->function, (unsigned)grid, 1, 1, 64, 1, 1, 0,
                                               (hipStream_t)stream, params, nullptr);
    return e == hipSuccess ? 0 : -2;
}

}  // namespace pcj
