// pc_io.cpp -- host ingest of FASTA/FASTQ(.gz) into the packed read arena the scan kernels consume
// (the row after the hot path) and the output writer (8f-3).  Pure host
// code, no GPU involved.
//
// Mirrors what the reference does between the file and the first alignment:
//   porechop/misc.py:60-81    get_compression_type  (gzip by magic bytes; bz2/zip refused)
//   porechop/misc.py:84-105   get_sequence_file_type ('>' FASTA, '@' FASTQ)
//   porechop/misc.py:123-148  load_fasta  (multi-line records, blank lines skipped, strip())
//   porechop/misc.py:151-168  load_fastq  (4 stripped lines per record)
//   porechop/nanopore_read.py:23-35  NanoporeRead.__init__ (upper(); U->T when U's outnumber T's;
//                                    qualities padded with '+')
// but produces one contiguous arena (1 byte per base, reads back to back, 64 bytes of 'N' padding
// at the end) plus offset/length tables -- exactly the inputs of pc_align_batch_host /
// pc_scan_device -- instead of millions of Python tuples.
//
// The writer (pc_readset_write) is the byte-level half of porechop/nanopore_read.py:97-147
// (get_fasta / get_fastq) and porechop/porechop.py:607-734 (output_reads): the caller decides WHICH
// pieces of which reads go to which file (trim amounts, split points, barcode bins -- integer
// arrays), this code formats them straight from the arena.
#include <zlib.h>

#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/uio.h>
#include <sys/statvfs.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <condition_variable>
#include <deque>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/porechop_amd.h"
#include "pc_gz.h"

// Byte buffers of the gzip reader: std::vector<char>::resize zeroes what it adds -- 32 MB per buffer the producer fills, 8 MB and
// more per member a worker inflates ahead -- before inflate overwrites every byte of it.  Default-initialising elements
// leaves the pages untouched until they are written.
template <class T> struct NoInitAlloc : std::allocator<T> {
    template <class U> struct rebind { using other = NoInitAlloc<U>; };
    NoInitAlloc() = default;
    template <class U> NoInitAlloc(const NoInitAlloc<U> &) {}
    template <class U> void construct(U *p) noexcept { ::new ((void *)p) U; }
    template <class U, class... A> void construct(U *p, A &&...a) { ::new ((void *)p) U(std::forward<A>(a)...); }
};
using Bytes = std::vector<char, NoInitAlloc<char>>;

// Big buffers are recycled: a streamed run loads and frees a read set per 256 MB block, and giving 128 MB back to
// the kernel and faulting 128 MB of fresh zeroed pages in again cost as much as writing the block (measured: 0.8 s of
// munmap per 6.4 GB run, as much again in page faults).  Freed buffers of 32 MB and more wait here (at most 3 GB) for
// the next request they fit.
namespace bigbuf {
struct Slot { char *p; size_t cap; };
inline std::mutex &mu() { static std::mutex m; return m; }
inline std::vector<Slot> &pool() { static std::vector<Slot> v; return v; }
inline size_t &held() { static size_t b = 0; return b; }
constexpr size_t kMin = (size_t)32 << 20, kMaxHeld = (size_t)3 << 30;
inline char *take(size_t want, size_t *cap)
{
    std::lock_guard<std::mutex> lk(mu());
    int best = -1;
    for (size_t i = 0; i < pool().size(); ++i)
        if (pool()[i].cap >= want && pool()[i].cap <= want * 3 && (best < 0 || pool()[i].cap < pool()[(size_t)best].cap)) best = (int)i;
    if (best < 0) return nullptr;
    const Slot s = pool()[(size_t)best];
    pool().erase(pool().begin() + best);
    held() -= s.cap;
    *cap = s.cap;
    return s.p;
}
inline bool give(char *p, size_t cap)
{
    if (!p || cap < kMin) return false;
    std::lock_guard<std::mutex> lk(mu());
    if (held() + cap > kMaxHeld) return false;
    pool().push_back({p, cap});
    held() += cap;
    return true;
}
}  // namespace bigbuf

// Growable byte buffer WITHOUT value-initialisation: the big arenas are sized once and filled by
// several threads; std::vector::resize would first zero gigabytes on one core.
struct RawBuf {
    char *p = nullptr;
    size_t n = 0, cap = 0;
    RawBuf() = default;
    RawBuf(const RawBuf &) = delete;
    RawBuf &operator=(const RawBuf &) = delete;
    ~RawBuf() { if (!bigbuf::give(p, cap)) free(p); }
    char *data() { return p; }
    const char *data() const { return p; }
    size_t size() const { return n; }
    void reserve(size_t c)
    {
        if (c <= cap) return;
        if (!p && c >= bigbuf::kMin) {                       // a first, large request: a recycled buffer if one fits
            size_t got = 0;
            if (char *q = bigbuf::take(c, &got)) { p = q; cap = got; return; }
        }
        size_t nc = cap ? cap : 4096;
        while (nc < c) nc += nc / 2 + 4096;
        char *q = (char *)realloc(p, nc);
        if (!q) abort();
        p = q; cap = nc;
    }
    void resize(size_t c) { reserve(c); n = c; }                       // new bytes are NOT initialised
    void append(const char *b, const char *e) { const size_t k = (size_t)(e - b); reserve(n + k); if (k) memcpy(p + n, b, k); n += k; }
    void fill(size_t k, char c) { reserve(n + k); memset(p + n, c, k); n += k; }
    void push_back(char c) { reserve(n + 1); p[n++] = c; }
    char &operator[](size_t i) { return p[i]; }
};

struct pc_readset {
    bool fastq = false;
    RawBuf arena;
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    std::vector<uint8_t> rna;
    // NUL-terminated strings back to back: read i's name at name_arena[name_off[i]], its qualities
    // (FASTQ only, padded with '+' to the sequence length) at qual_arena[qual_off[i]]
    RawBuf name_arena, qual_arena;
    std::vector<int64_t> name_off, qual_off;
    const char *name_of(size_t i) const { return name_arena.data() + name_off[i]; }
    size_t name_len(size_t i) const { return strlen(name_of(i)); }
    const char *qual_of(size_t i) const { return qual_arena.data() + qual_off[i]; }
    std::vector<int32_t> file_index;     // which input file a read came from (pc_readset_load_many)
    std::string error;
};

// What pc_readset_compress makes: per file, the compressed members of every formatter thread's span, in order.
struct pc_gzimage {
    std::vector<std::vector<std::vector<char>>> parts;      // [file][span]
    std::vector<int64_t> plain;                             // uncompressed bytes per file
    int64_t bytes(size_t f) const { int64_t b = 0; for (const auto &v : parts[f]) b += (int64_t)v.size(); return b; }
};

namespace {

// The bytes of a file: plain files are mapped (no copy), gzip files are inflated into memory.
struct FileData {
    const char *p = nullptr;
    size_t n = 0;
    void *map = nullptr;
    size_t map_len = 0;
    RawBuf owned;
    FileData() = default;
    FileData(const FileData &) = delete;
    ~FileData() { if (map) munmap(map, map_len); }
    const char *data() const { return p; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
};

int usable_threads();

// A gzip file made of members that carry their own size (pc_gz.h: what this library writes, and bgzip): the members are
// found by hopping from header to header and inflated by all cores, each into its place.  false = not such a file (or a
// member that does not check out): the caller inflates it as an ordinary gzip stream.
bool inflate_sized_members(const char *path, RawBuf &out)
{
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < (off_t)(pcz::kHeader + pcz::kTrailer)) { close(fd); return false; }
    const size_t size = (size_t)st.st_size;
    void *m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return false;
    const unsigned char *base = (const unsigned char *)m;
    struct Member { size_t in, in_n, out, out_n; uint32_t crc; };
    std::vector<Member> mem;
    size_t at = 0, total = 0;
    bool ok = true;
    while (at < size) {
        size_t payload = 0;
        const size_t n = pcz::sized_member(base + at, size - at, &payload);
        if (!n) { ok = false; break; }
        const size_t isize = pcz::get32(base + at + n - 4);
        mem.push_back({at + payload, n - payload - pcz::kTrailer, total, isize, pcz::get32(base + at + n - 8)});
        total += isize;
        at += n;
    }
    if (ok) {
        out.resize(total);
        const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)usable_threads(), mem.size() / 64 + 1));
        std::atomic<size_t> next{0};
        std::atomic<bool> good{true};
        auto work = [&]() {
            pcz::Inflater inf;
            for (;;) {
                const size_t i0 = next.fetch_add(64);
                if (i0 >= mem.size() || !good.load()) return;
                for (size_t i = i0; i < std::min(mem.size(), i0 + 64); ++i)
                    if (!inf.raw(base + mem[i].in, mem[i].in_n, out.data() + mem[i].out, mem[i].out_n, mem[i].crc)) { good.store(false); return; }
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back(work);
        work();
        for (auto &x : th) x.join();
        ok = good.load();
    }
    munmap(m, size);
    return ok;
}

// Any other gzip file, whole: the producer of the streamed route (gz_produce below) drained into one buffer -- members that
// were `cat`-ed together are inflated ahead by several cores, zero padding between and after members is skipped (as Python's
// gzip module, the reference's reader, does), and a stream that ends inside a member or is followed by anything else is an
// ERROR (zlib's gzread, used here before, returned what it had and said nothing: a truncated download lost reads silently,
// where the reference stops with an exception).
bool inflate_whole_gzip(const char *path, RawBuf &out);

bool slurp(const char *path, FileData &data, std::string &err)
{
    FILE *f = fopen(path, "rb");
    if (!f) { err = std::string("could not find ") + path; return false; }
    unsigned char magic[4] = {0, 0, 0, 0};
    const size_t got = fread(magic, 1, 4, f);
    fclose(f);
    if (got >= 3 && magic[0] == 0x42 && magic[1] == 0x5a && magic[2] == 0x68) { err = "cannot use bzip2 format - use gzip instead"; return false; }
    if (got >= 4 && magic[0] == 0x50 && magic[1] == 0x4b && magic[2] == 0x03 && magic[3] == 0x04) { err = "cannot use zip format - use gzip instead"; return false; }
    // gzopen reads plain files transparently, but the reference decides by magic bytes: do the same
    const bool gz = got >= 3 && magic[0] == 0x1f && magic[1] == 0x8b && magic[2] == 0x08;
    if (gz && inflate_sized_members(path, data.owned)) {
        data.p = data.owned.data(); data.n = data.owned.size();
    } else if (gz) {
        if (!inflate_whole_gzip(path, data.owned)) { err = "gzip stream error (damaged, or ended before the end of a member)"; return false; }
        data.p = data.owned.data(); data.n = data.owned.size();
    } else {
        const int fd = open(path, O_RDONLY);
        if (fd < 0) { err = std::string("could not open ") + path; return false; }
        struct stat st;
        if (fstat(fd, &st) != 0) { err = std::string("could not open ") + path; close(fd); return false; }
        if (st.st_size > 0) {
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) {                               // e.g. a pipe: read it
                data.owned.resize((size_t)st.st_size);
                size_t have = 0;
                while (have < data.owned.size()) {
                    const ssize_t k = read(fd, data.owned.data() + have, data.owned.size() - have);
                    if (k <= 0) break;
                    have += (size_t)k;
                }
                data.owned.resize(have);
                data.p = data.owned.data(); data.n = have;
            } else {
                madvise(m, (size_t)st.st_size, MADV_WILLNEED);
                data.map = m; data.map_len = (size_t)st.st_size;
                data.p = (const char *)m; data.n = (size_t)st.st_size;
            }
        }
        close(fd);
    }
    return true;
}

// Python str.strip(): ASCII whitespace on both sides
inline void strip(const char *&b, const char *&e)
{
    while (b < e && isspace((unsigned char)*b)) ++b;
    while (e > b && isspace((unsigned char)e[-1])) --e;
}

struct Lines {
    const char *p, *end;
    bool next(const char *&b, const char *&e)
    {
        if (p >= end) return false;
        b = p;
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        e = nl ? nl : end;
        p = nl ? nl + 1 : end;
        return true;
    }
};

struct UpperTable {
    unsigned char t[256];
    UpperTable() { for (int i = 0; i < 256; ++i) t[i] = (unsigned char)((i >= 'a' && i <= 'z') ? i - 32 : i); }
};
const UpperTable kUpper;

// NanoporeRead.__init__ (nanopore_read.py:23-35) on one read: upper-case copy + the counts of 'U' and 'T' that decide
// whether it is RNA.  Arithmetic instead of a table, so that the loop vectorises (the table form ran at ~1.5 GB/s per
// core and was most of the parser's second pass).
__attribute__((target_clones("avx2", "default")))
void upper_copy_count(unsigned char *__restrict dst, const unsigned char *__restrict src, size_t n, size_t *nu_out, size_t *nt_out)
{
    size_t nu = 0, nt = 0;
    size_t i = 0;
    while (i < n) {
        const size_t stop = n - i > 240 ? i + 240 : n;        // byte-wide partial counts cannot overflow within 240 bases
        unsigned char u8 = 0, t8 = 0;
        for (; i < stop; ++i) {
            unsigned char c = src[i];
            c = (unsigned char)(c - (((unsigned char)(c - 'a') < 26) ? 32 : 0));
            dst[i] = c;
            u8 = (unsigned char)(u8 + (c == 'U'));
            t8 = (unsigned char)(t8 + (c == 'T'));
        }
        nu += u8; nt += t8;
    }
    *nu_out = nu; *nt_out = nt;
}

void add_read(pc_readset *rs, const char *name_b, const char *name_e, const char *seq_b, const char *seq_e,
              const char *q_b, const char *q_e)
{
    // NanoporeRead.__init__: upper(); if count('U') > count('T'): U -> T
    const size_t n = (size_t)(seq_e - seq_b);
    const size_t o = rs->arena.size();
    rs->arena.resize(o + n);
    unsigned char *dst = (unsigned char *)rs->arena.data() + o;
    size_t nu = 0, nt = 0;
    upper_copy_count(dst, (const unsigned char *)seq_b, n, &nu, &nt);
    const bool rna = nu > nt;
    if (rna) for (size_t i = 0; i < n; ++i) if (dst[i] == 'U') dst[i] = 'T';
    rs->off.push_back((int64_t)o);
    rs->len.push_back((int32_t)n);
    rs->rna.push_back(rna ? 1 : 0);
    rs->name_off.push_back((int64_t)rs->name_arena.size());
    rs->name_arena.append(name_b, name_e);
    rs->name_arena.push_back('\0');
    if (rs->fastq) {
        rs->qual_off.push_back((int64_t)rs->qual_arena.size());
        rs->qual_arena.append(q_b, q_e);
        const size_t ql = (size_t)(q_e - q_b);
        if (ql < n) rs->qual_arena.fill(n - ql, '+');
        rs->qual_arena.push_back('\0');
    }
}

thread_local int t_thread_limit = 0;      // pc_io_set_thread_limit: this caller thread's share of the host cores

int usable_threads()
{
    if (t_thread_limit > 0) return t_thread_limit;
    cpu_set_t set;
    int n = 0;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = (int)std::thread::hardware_concurrency();
    // a container's CPU quota (cgroup v2 cpu.max "quota period"): more runnable threads than that only buy throttling --
    // the GPU box shows 256 CPUs in its affinity mask and a quota of 16
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        long period = 0;
        if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            const long quota = atol(q);
            if (quota > 0) n = std::min<long>(n, std::max<long>(1, (quota + period - 1) / period));
        }
        fclose(f);
    }
    if (const char *e = getenv("PC_IO_THREADS")) { const int v = atoi(e); if (v > 0) n = v; }
    return std::max(1, std::min(n, 64));
}

// ---- parallel FASTQ parse ---------------------------------------------------------------------
// The reference's loader takes FASTQ strictly as 4 stripped lines per record (misc.py:151-168).
// A record start is therefore a line beginning with '@' whose next-but-one line begins with '+':
// a quality line may begin with '@', but then the line two below it is a sequence line, never '+'.
// The file is cut at such boundaries into one span per thread; pass 1 sizes every span, a prefix
// sum places it, pass 2 writes reads straight into their final position.  Anything irregular
// (missing lines, blank lines, a header that is not '@') is left to the serial parser, which
// reproduces the reference's behaviour and error messages for those cases.
struct Span { const char *b, *e; size_t reads = 0, seq = 0, name = 0, qual = 0; bool ok = true; };

inline const char *line_end(const char *p, const char *end) { const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p)); return nl ? nl : end; }
inline const char *next_line(const char *p, const char *end) { const char *nl = line_end(p, end); return nl < end ? nl + 1 : end; }

const char *find_record_start(const char *p, const char *begin, const char *end)
{
    if (p <= begin) return begin;
    p = next_line(p - 1, end);                                   // first line start at or after p
    for (int tries = 0; tries < 8 && p < end; ++tries) {
        const char *l2 = next_line(next_line(p, end), end);
        if (*p == '@' && l2 < end && *l2 == '+') return p;
        p = next_line(p, end);
    }
    return nullptr;                                               // not a regular 4-line FASTQ around here
}

template <class Fn> bool for_each_record(const Span &sp, Fn fn)
{
    const char *p = sp.b;
    while (p < sp.e) {
        const char *b0 = p, *e0 = line_end(p, sp.e);
        if (e0 >= sp.e) return false;                             // a record needs four lines
        const char *b1 = e0 + 1, *e1 = line_end(b1, sp.e);
        if (e1 >= sp.e) return false;
        const char *b2 = e1 + 1, *e2 = line_end(b2, sp.e);
        if (e2 >= sp.e) return false;
        const char *b3 = e2 + 1, *e3 = line_end(b3, sp.e);
        if (b3 >= sp.e) return false;
        const char *nb = b0, *ne = e0;
        strip(nb, ne);
        if (nb == ne || *nb != '@' || *b2 != '+') return false;
        ++nb;
        if (nb == ne) return false;                               // empty name: the reference fails on it
        const char *sb = b1, *se = e1, *qb = b3, *qe = e3;
        strip(sb, se); strip(qb, qe);
        fn(nb, ne, sb, se, qb, qe);
        p = e3 < sp.e ? e3 + 1 : sp.e;
    }
    return true;
}

bool parse_fastq_range(pc_readset *rs, const char *begin, const char *end, int nthreads)
{
    std::vector<Span> spans;
    const char *prev = begin;
    const size_t size = (size_t)(end - begin);
    for (int t = 1; t <= nthreads; ++t) {
        const char *cut = t == nthreads ? end : find_record_start(begin + size / (size_t)nthreads * (size_t)t, begin, end);
        if (!cut) cut = end;             // no record start found from there on (a long last record, or an irregular file:
                                         // the record walk below rejects those): the rest is one span
        if (cut > prev) { Span sp; sp.b = prev; sp.e = cut; spans.push_back(sp); prev = cut; }
    }
    auto run = [&](auto fn) {
        std::vector<std::thread> th;
        for (size_t k = 1; k < spans.size(); ++k) th.emplace_back(fn, k);
        fn((size_t)0);
        for (auto &x : th) x.join();
    };
    run([&](size_t k) {
        Span &sp = spans[k];
        sp.ok = for_each_record(sp, [&](const char *nb, const char *ne, const char *sb, const char *se, const char *qb, const char *qe) {
            const size_t n = (size_t)(se - sb), q = (size_t)(qe - qb);
            ++sp.reads; sp.seq += n; sp.name += (size_t)(ne - nb) + 1; sp.qual += std::max(n, q) + 1;
        });
    });
    for (const Span &sp : spans) if (!sp.ok) return false;
    // placement
    const size_t r0 = rs->off.size(), s0 = rs->arena.size(), n0 = rs->name_arena.size(), q0 = rs->qual_arena.size();
    std::vector<size_t> rb(spans.size() + 1, r0), sb_(spans.size() + 1, s0), nb_(spans.size() + 1, n0), qb_(spans.size() + 1, q0);
    for (size_t k = 0; k < spans.size(); ++k) {
        rb[k + 1] = rb[k] + spans[k].reads; sb_[k + 1] = sb_[k] + spans[k].seq;
        nb_[k + 1] = nb_[k] + spans[k].name; qb_[k + 1] = qb_[k] + spans[k].qual;
    }
    rs->off.resize(rb.back()); rs->len.resize(rb.back()); rs->rna.resize(rb.back());
    rs->name_off.resize(rb.back()); rs->qual_off.resize(rb.back());
    rs->arena.resize(sb_.back()); rs->name_arena.resize(nb_.back()); rs->qual_arena.resize(qb_.back());
    run([&](size_t k) {
        size_t r = rb[k], so = sb_[k], no = nb_[k], qo = qb_[k];
        for_each_record(spans[k], [&](const char *nb, const char *ne, const char *sb, const char *se, const char *qb, const char *qe) {
            const size_t n = (size_t)(se - sb), q = (size_t)(qe - qb);
            unsigned char *dst = (unsigned char *)rs->arena.data() + so;
            size_t nu = 0, nt = 0;
            upper_copy_count(dst, (const unsigned char *)sb, n, &nu, &nt);
            const bool rna = nu > nt;
            if (rna) for (size_t i = 0; i < n; ++i) if (dst[i] == 'U') dst[i] = 'T';
            rs->off[r] = (int64_t)so; rs->len[r] = (int32_t)n; rs->rna[r] = rna ? 1 : 0;
            rs->name_off[r] = (int64_t)no;
            memcpy(rs->name_arena.data() + no, nb, (size_t)(ne - nb));
            rs->name_arena[no + (size_t)(ne - nb)] = '\0';
            rs->qual_off[r] = (int64_t)qo;
            memcpy(rs->qual_arena.data() + qo, qb, q);
            if (q < n) memset(rs->qual_arena.data() + qo + q, '+', n - q);
            rs->qual_arena[qo + std::max(n, q)] = '\0';
            ++r; so += n; no += (size_t)(ne - nb) + 1; qo += std::max(n, q) + 1;
        });
    });
    return true;
}

bool parse_fastq_parallel(pc_readset *rs, const FileData &data, int nthreads)
{
    return parse_fastq_range(rs, data.data(), data.data() + data.size(), nthreads);
}

}  // namespace

extern "C" {

// parse one file into rs (reads appended); rs->fastq is set by the first file
// FASTA, the reference's way (misc.py:123-148), on one span: lines stripped, blank lines skipped, a stripped line that starts
// with '>' opens a record, everything else is appended to the running sequence.  A record whose name is empty is not kept --
// and, as there, its sequence is NOT cleared when the next header comes (`sequence = ''` sits under `if name:`), so it ends
// up in front of the next named record's.  *carry_out = what a span that ends inside such a nameless record would hand on.
static void parse_fasta_span(pc_readset *rs, const char *begin, const char *end, std::string *carry_out = nullptr)
{
    Lines ln{begin, end};
    const char *b, *e;
    std::string name, seq;
    while (ln.next(b, e)) {
        strip(b, e);
        if (b == e) continue;
        if (*b == '>') {
            if (!name.empty()) {
                add_read(rs, name.data(), name.data() + name.size(), seq.data(), seq.data() + seq.size(), nullptr, nullptr);
                seq.clear();
            }
            name.assign(b + 1, e);
        } else {
            seq.append(b, e);
        }
    }
    if (!name.empty()) { add_read(rs, name.data(), name.data() + name.size(), seq.data(), seq.data() + seq.size(), nullptr, nullptr); seq.clear(); }
    if (carry_out) *carry_out = seq;
}

// The same on all cores: the file is cut where a line BEGINS with '>' (such a line opens a record whatever the stripping does;
// a header with blanks in front of its '>' simply stays inside a span), every span is parsed by the serial rule into its own
// read set, and the sets are appended in order.  false (nothing added): a span ends inside a nameless record whose sequence the
// next span's first record would inherit -- the caller parses the file serially.
static bool parse_fasta_parallel(pc_readset *rs, const char *begin, const char *end, int nthreads, std::string *last_carry = nullptr)
{
    const size_t size = (size_t)(end - begin);
    std::vector<const char *> cut{begin};
    for (int t = 1; t < nthreads; ++t) {
        const char *p = begin + size / (size_t)nthreads * (size_t)t;
        if (p <= cut.back()) continue;
        const char *q = nullptr;
        for (const char *s = p; s + 1 < end; ) {
            const char *nl = (const char *)memchr(s, '\n', (size_t)(end - 1 - s));
            if (!nl) break;
            if (nl[1] == '>') { q = nl + 1; break; }
            s = nl + 1;
        }
        if (!q) break;
        if (q > cut.back()) cut.push_back(q);
    }
    cut.push_back(end);
    const size_t nspans = cut.size() - 1;
    std::vector<std::unique_ptr<pc_readset>> part(nspans);
    std::vector<std::string> carry(nspans);
    std::vector<std::thread> th;
    auto work = [&](size_t k) {
        part[k].reset(new pc_readset());
        part[k]->arena.reserve((size_t)(cut[k + 1] - cut[k]) + 64);
        parse_fasta_span(part[k].get(), cut[k], cut[k + 1], &carry[k]);
    };
    for (size_t k = 1; k < nspans; ++k) th.emplace_back(work, k);
    work(0);
    for (auto &x : th) x.join();
    for (size_t k = 0; k + 1 < nspans; ++k) if (!carry[k].empty()) return false;
    if (last_carry) *last_carry = carry[nspans - 1];
    // every span's reads go to their place side by side (the copies are also the first touch of the big arena's pages)
    std::vector<size_t> r0(nspans + 1, rs->off.size()), a0(nspans + 1, rs->arena.size()), n0(nspans + 1, rs->name_arena.size());
    for (size_t k = 0; k < nspans; ++k) {
        r0[k + 1] = r0[k] + part[k]->off.size();
        a0[k + 1] = a0[k] + part[k]->arena.size();
        n0[k + 1] = n0[k] + part[k]->name_arena.size();
    }
    rs->arena.reserve(a0[nspans] + 128);
    rs->arena.resize(a0[nspans]);
    rs->name_arena.resize(n0[nspans]);
    rs->off.resize(r0[nspans]); rs->len.resize(r0[nspans]); rs->rna.resize(r0[nspans]); rs->name_off.resize(r0[nspans]);
    auto place = [&](size_t k) {
        pc_readset &p = *part[k];
        if (p.arena.size()) memcpy(rs->arena.data() + a0[k], p.arena.data(), p.arena.size());
        if (p.name_arena.size()) memcpy(rs->name_arena.data() + n0[k], p.name_arena.data(), p.name_arena.size());
        for (size_t i = 0; i < p.off.size(); ++i) {
            rs->off[r0[k] + i] = (int64_t)a0[k] + p.off[i];
            rs->name_off[r0[k] + i] = (int64_t)n0[k] + p.name_off[i];
            rs->len[r0[k] + i] = p.len[i];
            rs->rna[r0[k] + i] = p.rna[i];
        }
        part[k].reset();
    };
    th.clear();
    for (size_t k = 1; k < nspans; ++k) th.emplace_back(place, k);
    place(0);
    for (auto &x : th) x.join();
    return true;
}

// ---- FASTA by segments (streamed / sharded runs; the FASTQ twins are find_record_start / parse_fastq_range) ------------
// A cut may fall wherever a line BEGINS with '>' (a header the reference only finds after stripping blanks is never
// used as a cut: it stays inside a segment, where the parser treats it as the reference does).
static const char *find_fasta_record_start(const char *p, const char *begin, const char *end)
{
    if (p <= begin) return begin;
    for (const char *s = p - 1; s < end; ) {
        const char *nl = (const char *)memchr(s, '\n', (size_t)(end - s));
        if (!nl || nl + 1 >= end) return nullptr;
        if (nl[1] == '>') return nl + 1;
        s = nl + 1;
    }
    return nullptr;
}
// The records of [begin, end), which starts with a header line.  false: the segment cannot stand alone -- its last header has an
// empty name, whose bases the reference hands on to the NEXT record (misc.py:123-148): the whole-file loader's case.
static bool parse_fasta_range(pc_readset *rs, const char *begin, const char *end, int nthreads, bool to_the_end)
{
    std::string carry;
    if ((size_t)(end - begin) >= ((size_t)1 << 20) && nthreads > 1 && parse_fasta_parallel(rs, begin, end, nthreads, &carry)) {
    } else {
        parse_fasta_span(rs, begin, end, &carry);               // (a refused parallel parse has not touched rs)
    }
    return to_the_end || carry.empty();
}

static int load_into(pc_readset *rs, const char *path, int32_t file_index, bool first, FileData *ready = nullptr,
                     const std::string *ready_error = nullptr)
{
    FileData own;
    if (ready && ready_error && !ready_error->empty()) { rs->error = *ready_error; return PC_ERR_BAD_ARG; }
    if (!ready && !slurp(path, own, rs->error)) return PC_ERR_BAD_ARG;
    FileData &data = ready ? *ready : own;
    const char first_char = data.empty() ? '\0' : data.data()[0];
    if (first_char != '>' && first_char != '@') { rs->error = "File is neither FASTA or FASTQ"; return PC_ERR_BAD_ARG; }
    const bool fastq = (first_char == '@');
    if (first) rs->fastq = fastq;
    else if (fastq != rs->fastq) { rs->error = std::string(path) + " is not of the same type as the files before it"; return PC_ERR_BAD_ARG; }
    rs->arena.reserve(rs->arena.size() + data.size() / (rs->fastq ? 2 : 1) + 128);
    const size_t before = rs->off.size();
    Lines ln{data.data(), data.data() + data.size()};
    const char *b, *e;
    static const bool serial_only = [] { const char *e = getenv("PC_IO_SERIAL"); return e && *e && *e != '0'; }();
    if (rs->fastq && !serial_only && data.size() >= ((size_t)1 << 20) && parse_fastq_parallel(rs, data, usable_threads())) {
        // regular 4-line FASTQ, parsed in parallel
    } else if (rs->fastq) {
        while (ln.next(b, e)) {
            strip(b, e);
            const char *nb = b < e ? b + 1 : b;           // line.strip()[1:]
            const char *sb, *se, *pb, *pe, *qb, *qe;
            if (nb == e || !ln.next(sb, se) || !ln.next(pb, pe) || !ln.next(qb, qe)) {
                rs->error = std::string(path) + " could not be parsed - is it formatted correctly?";
                return PC_ERR_BAD_ARG;
            }
            strip(sb, se); strip(qb, qe);
            add_read(rs, nb, e, sb, se, qb, qe);
        }
    } else if (!serial_only && data.size() >= ((size_t)1 << 20) && usable_threads() > 1 &&
               parse_fasta_parallel(rs, data.data(), data.data() + data.size(), usable_threads())) {
        // FASTA, parsed in parallel
    } else {
        parse_fasta_span(rs, data.data(), data.data() + data.size());
    }
    rs->file_index.resize(rs->off.size(), file_index);
    (void)before;
    return PC_OK;
}

int pc_readset_load_many(const char *const *paths, int npaths, pc_readset **out)
{
    if (!paths || npaths < 1 || !out) return PC_ERR_BAD_ARG;
    pc_readset *rs = new pc_readset();
    *out = rs;
    // Several files (an Albacore / Guppy directory: thousands of .fastq.gz of a few thousand reads each,
    // porechop.py:216-268): the files of a batch are read -- and inflated -- side by side, one thread each, then parsed in
    // order (what a file's error is, and which file reports first, stay the reference's: errors are kept per file and raised
    // at the file's turn).  One file: as before (its own inflate / parse use all cores).
    const int T = npaths > 1 ? usable_threads() : 1;
    for (int i0 = 0; i0 < npaths; i0 += T) {
        const int i1 = std::min(npaths, i0 + T);
        if (i1 - i0 == 1) {
            const int rc = load_into(rs, paths[i0], i0, i0 == 0);
            if (rc) return rc;
            continue;
        }
        std::vector<FileData> data((size_t)(i1 - i0));
        std::vector<std::string> errs((size_t)(i1 - i0));
        std::vector<std::thread> th;
        const int limit = t_thread_limit;
        for (int i = i0; i < i1; ++i)
            th.emplace_back([&, i] {
                t_thread_limit = 1;                       // (this file's share: the batch is the parallelism)
                std::string e;
                if (!slurp(paths[i], data[(size_t)(i - i0)], e)) errs[(size_t)(i - i0)] = e.empty() ? std::string("could not open ") + paths[i] : e;
            });
        for (auto &x : th) x.join();
        t_thread_limit = limit;
        for (int i = i0; i < i1; ++i) {
            const int rc = load_into(rs, paths[i], i, i == 0, &data[(size_t)(i - i0)], &errs[(size_t)(i - i0)]);
            if (rc) return rc;
        }
    }
    rs->arena.fill(64, 'N');                              // the kernels fetch a dword at a time
    return PC_OK;
}

int pc_readset_load(const char *path, pc_readset **out)
{
    if (!path || !out) return PC_ERR_BAD_ARG;
    return pc_readset_load_many(&path, 1, out);
}

// One segment of a plain, regular 4-line FASTQ file -- or of a plain FASTA file, cut where a line begins with '>' -- : the
// records that START in [byte_begin, cut), cut = the first record start at or after byte_begin + target_bytes (or the end
// of the file).  *next_begin = cut (== the file size after the last segment).  PC_ERR_UNSUPPORTED_SCORES is (re)used as
// "not streamable" (gzip, an irregular FASTQ record, a FASTA segment that ends in a header without a name -- its bases
// belong to the next record): the caller then loads the whole file with pc_readset_load, which reproduces the reference's
// behaviour and messages for those inputs.
int pc_readset_load_segment(const char *path, int64_t byte_begin, int64_t target_bytes, int64_t *next_begin, pc_readset **out)
{
    if (!path || !out || !next_begin || byte_begin < 0 || target_bytes <= 0) return PC_ERR_BAD_ARG;
    pc_readset *rs = new pc_readset();
    *out = rs;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) { rs->error = std::string("could not find ") + path; return PC_ERR_BAD_ARG; }
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size <= 0 || byte_begin > (int64_t)st.st_size) { close(fd); rs->error = "not streamable"; return PC_ERR_UNSUPPORTED_SCORES; }
    const size_t size = (size_t)st.st_size;
    void *m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) { rs->error = "not streamable"; return PC_ERR_UNSUPPORTED_SCORES; }
    const char *base = (const char *)m, *fend = base + size;
    int rc = PC_OK;
    const bool fasta = base[0] == '>';
    if (base[0] != '@' && !fasta) rc = PC_ERR_UNSUPPORTED_SCORES;   // gzip, ...: neither a plain FASTQ nor a plain FASTA
    const char *b = base + byte_begin, *e = fend;
    if (rc == PC_OK && fasta && b < fend) {
        if (*b != '>') rc = PC_ERR_UNSUPPORTED_SCORES;              // (a segment starts at a cut: a header line)
        if (rc == PC_OK && (size_t)(fend - b) > (size_t)target_bytes) {
            e = find_fasta_record_start(b + target_bytes, b, fend);
            if (!e) e = fend;                                       // no header after the target: the file's last record
        }
        if (rc == PC_OK) {
            rs->fastq = false;
            // a segment that ends in a header without a name cannot stand alone (its bases go to the NEXT record): it is
            // extended header by header until it can, or to the end of the file -- never refused in mid-stream
            while (e > b && !parse_fasta_range(rs, b, e, usable_threads(), e == fend)) {
                const char *nx = e < fend ? find_fasta_record_start(e + 1, b, fend) : nullptr;
                e = nx ? nx : fend;
                delete rs;
                rs = new pc_readset();
                *out = rs;
                rs->fastq = false;
            }
        }
    } else if (rc == PC_OK && b < fend) {
        if ((size_t)(fend - b) > (size_t)target_bytes) {
            e = find_record_start(b + target_bytes, b, fend);
            if (!e) {
                // no record starts after the target: the file's last record (fewer than eight lines remain), or irregular
                const char *q = next_line(b + target_bytes - 1, fend);
                for (int tries = 0; tries < 8 && q < fend; ++tries) q = next_line(q, fend);
                if (q >= fend) e = fend; else rc = PC_ERR_UNSUPPORTED_SCORES;
            }
        }
        if (rc == PC_OK) {
            {
                const size_t first = (size_t)(b - base) & ~(size_t)4095;
                madvise((void *)(base + first), (size_t)(e - base) - first, MADV_WILLNEED);
            }
            rs->fastq = true;
            if (e > b && !parse_fastq_range(rs, b, e, usable_threads())) rc = PC_ERR_UNSUPPORTED_SCORES;
        }
    }
    if (rc == PC_OK) {
        rs->file_index.resize(rs->off.size(), 0);
        rs->arena.fill(64, 'N');
        *next_begin = (int64_t)(e - base);
    } else {
        rs->error = "not streamable";
    }
    munmap(m, size);
    return rc;
}

// The first record start at or after byte_pos of a plain 4-line FASTQ file -- the `cut` pc_readset_load_segment would
// choose for byte_begin + target_bytes == byte_pos -- or the file's size when no record starts there any more.  Lets the
// ranks of a sharded run find their own byte ranges without reading anything else of the file.
int pc_fastq_find_record(const char *path, int64_t byte_pos, int64_t *record_start)
{
    if (!path || !record_start || byte_pos < 0) return PC_ERR_BAD_ARG;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return PC_ERR_BAD_ARG;
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size <= 0) { close(fd); return PC_ERR_UNSUPPORTED_SCORES; }
    const size_t size = (size_t)st.st_size;
    if ((size_t)byte_pos >= size) { close(fd); *record_start = (int64_t)size; return PC_OK; }
    void *m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return PC_ERR_UNSUPPORTED_SCORES;
    const char *base = (const char *)m, *fend = base + size;
    int rc = PC_OK;
    if (base[0] == '>') {                                            // FASTA: the next line that begins with '>' (or the end)
        const char *e = find_fasta_record_start(base + byte_pos, base, fend);
        *record_start = (int64_t)((e ? e : fend) - base);
        munmap(m, size);
        return PC_OK;
    }
    if (base[0] != '@') rc = PC_ERR_UNSUPPORTED_SCORES;
    if (rc == PC_OK) {
        const char *e = find_record_start(base + byte_pos, base, fend);
        if (!e) {
            const char *q = next_line(base + byte_pos - 1, fend);
            for (int tries = 0; tries < 8 && q < fend; ++tries) q = next_line(q, fend);
            if (q >= fend) e = fend; else rc = PC_ERR_UNSUPPORTED_SCORES;
        }
        if (rc == PC_OK) *record_start = (int64_t)(e - base);
    }
    munmap(m, size);
    return rc;
}

// ---- a gzip FASTQ file of SIZED members, addressed by positions in its inflated bytes (sharded runs) ------------------
// Members that carry their size (what this library writes; bgzip) are independent and found by hopping from header to
// header: the inflated stream can be addressed like a plain file without inflating it -- position x lies in the member whose
// inflated span holds it.  That gives the ranks of a sharded run what pc_fastq_find_record / pc_readset_load_segment give
// them on a plain file: rank r of W takes the records that start in [find(total * r / W), find(total * (r + 1) / W)) of
// the inflated bytes and inflates only the members that hold them.
namespace {
struct SizedIndex {
    struct M { size_t in, in_n, out, out_n; uint32_t crc; };
    const unsigned char *base = nullptr;
    size_t size = 0, total = 0;
    std::vector<M> mem;
    ~SizedIndex() { if (base) munmap((void *)base, size); }
    // false: not a file made of sized members from its first byte to its last
    bool open_file(const char *path)
    {
        const int fd = open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || st.st_size < (off_t)(pcz::kHeader + pcz::kTrailer)) { close(fd); return false; }
        size = (size_t)st.st_size;
        void *m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (m == MAP_FAILED) { size = 0; return false; }
        base = (const unsigned char *)m;
        size_t at = 0;
        while (at < size) {
            size_t payload = 0;
            const size_t n = pcz::sized_member(base + at, size - at, &payload);
            if (!n) return false;
            const size_t isize = pcz::get32(base + at + n - 4);
            mem.push_back({at + payload, n - payload - pcz::kTrailer, total, isize, pcz::get32(base + at + n - 8)});
            total += isize;
            at += n;
        }
        return true;
    }
    // the member that holds inflated position x (x < total); empty members are skipped over
    size_t member_of(size_t x) const
    {
        size_t lo = 0, hi = mem.size();
        while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (mem[mid].out <= x) lo = mid; else hi = mid; }
        return lo;
    }
    // inflates the members that hold [a, b) (a < b <= total) -> buf holds the inflated bytes from *buf_at on
    bool inflate(size_t a, size_t b, RawBuf &buf, size_t *buf_at) const
    {
        const size_t m0 = member_of(a), m1 = member_of(b - 1) + 1;
        const size_t o0 = mem[m0].out, o1 = mem[m1 - 1].out + mem[m1 - 1].out_n;
        buf.resize(o1 - o0);
        *buf_at = o0;
        const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)usable_threads(), (m1 - m0) / 64 + 1));
        std::atomic<size_t> next{m0};
        std::atomic<bool> good{true};
        auto work = [&]() {
            pcz::Inflater inf;
            for (;;) {
                const size_t i0 = next.fetch_add(64);
                if (i0 >= m1 || !good.load()) return;
                for (size_t i = i0; i < std::min(m1, i0 + 64); ++i)
                    if (!inf.raw(base + mem[i].in, mem[i].in_n, buf.data() + (mem[i].out - o0), mem[i].out_n, mem[i].crc)) { good.store(false); return; }
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back(work);
        work();
        for (auto &x : th) x.join();
        return good.load();
    }
};
}  // namespace

// The inflated size of a gzip file made of sized members only; PC_ERR_UNSUPPORTED_SCORES for any other file.
int pc_gz_sized_size(const char *path, int64_t *inflated_bytes)
{
    if (!path || !inflated_bytes) return PC_ERR_BAD_ARG;
    SizedIndex ix;
    if (!ix.open_file(path)) return PC_ERR_UNSUPPORTED_SCORES;
    *inflated_bytes = (int64_t)ix.total;
    return PC_OK;
}

// pc_fastq_find_record on the inflated bytes of such a file: the first record start at or after `pos`, or the inflated size
// when none is left.  Only the members around `pos` are inflated (a window that doubles until the record start is found).
int pc_gz_sized_find_record(const char *path, int64_t pos, int64_t *record_start)
{
    if (!path || !record_start || pos < 0) return PC_ERR_BAD_ARG;
    SizedIndex ix;
    if (!ix.open_file(path) || ix.total == 0) return PC_ERR_UNSUPPORTED_SCORES;
    if ((size_t)pos >= ix.total) { *record_start = (int64_t)ix.total; return PC_OK; }
    if (pos == 0) { *record_start = 0; return PC_OK; }
    // FASTQ or FASTA: the stream's first byte says (a FASTA stream is cut where a line begins with '>')
    bool fasta = false;
    {
        RawBuf head;
        size_t head_at = 0;
        if (!ix.inflate(0, 1, head, &head_at) || head.size() == 0) return PC_ERR_UNSUPPORTED_SCORES;
        fasta = head.data()[0] == '>';
        if (!fasta && head.data()[0] != '@') return PC_ERR_UNSUPPORTED_SCORES;
    }
    const size_t x = (size_t)pos;
    for (size_t window = (size_t)1 << 20; ; window *= 4) {
        const size_t b = std::min(ix.total, x + window);
        RawBuf buf;
        size_t buf_at = 0;
        if (!ix.inflate(x - 1, b, buf, &buf_at)) return PC_ERR_UNSUPPORTED_SCORES;
        const char *wb = buf.data(), *we = buf.data() + buf.size(), *p = wb + (x - buf_at);
        const bool to_the_end = buf_at + buf.size() >= ix.total;
        if (fasta) {
            const char *e = find_fasta_record_start(p, wb, we);
            if (e) { *record_start = (int64_t)(buf_at + (size_t)(e - wb)); return PC_OK; }
            if (to_the_end) { *record_start = (int64_t)ix.total; return PC_OK; }
            continue;
        }
        // (p > wb unless the window starts at the stream's first byte, where find_record_start's `begin` shortcut is right)
        const char *e = find_record_start(p, wb, we);
        if (e) {
            // final: it was judged by lines inside the window, and so was every line start before it (a candidate is only
            // passed over for want of bytes when its '+' line lies beyond the window -- then so does every later one's)
            *record_start = (int64_t)(buf_at + (size_t)(e - wb));
            return PC_OK;
        }
        if (to_the_end) {
            // no record starts after pos: the stream's last record (fewer than eight lines remain), or irregular
            const char *q = next_line(p - 1, we);
            for (int tries = 0; tries < 8 && q < we; ++tries) q = next_line(q, we);
            if (q >= we) { *record_start = (int64_t)ix.total; return PC_OK; }
            return PC_ERR_UNSUPPORTED_SCORES;
        }
    }
}

// The records of [begin, end) of the inflated bytes -- both record starts as pc_gz_sized_find_record gives them (or the
// inflated size) -- as a read set: pc_readset_load_segment for one rank's share of such a file.
int pc_readset_load_gz_range(const char *path, int64_t begin, int64_t end, pc_readset **out)
{
    if (!path || !out || begin < 0 || end < begin) return PC_ERR_BAD_ARG;
    pc_readset *rs = new pc_readset();
    *out = rs;
    rs->fastq = true;
    SizedIndex ix;
    if (!ix.open_file(path) || (size_t)end > ix.total) { rs->error = "not streamable"; return PC_ERR_UNSUPPORTED_SCORES; }
    if (end > begin) {
        RawBuf buf;
        size_t buf_at = 0;
        if (!ix.inflate((size_t)begin, (size_t)end, buf, &buf_at)) { rs->error = "gzip stream error"; return PC_ERR_UNSUPPORTED_SCORES; }
        const char *b = buf.data() + ((size_t)begin - buf_at), *e = buf.data() + ((size_t)end - buf_at);
        if (*b == '>') {
            // FASTA: a share that ends in a header without a name cannot stand alone (its bases belong to the next rank's first
            // record): not this route -- the caller gathers
            rs->fastq = false;
            if (!parse_fasta_range(rs, b, e, usable_threads(), (size_t)end >= ix.total)) { rs->error = "not streamable"; return PC_ERR_UNSUPPORTED_SCORES; }
        } else if (*b != '@' || !parse_fastq_range(rs, b, e, usable_threads())) { rs->error = "not streamable"; return PC_ERR_UNSUPPORTED_SCORES; }
    }
    rs->file_index.resize(rs->off.size(), 0);
    rs->arena.fill(64, 'N');
    return PC_OK;
}

// ---- a gzip FASTQ file as a stream of blocks (the streamed route of runner.py for .gz input) -------------------------
// A producer thread inflates AHEAD of the consumer into a bounded queue of buffers: members that carry their size
// (pc_gz.h) a batch at a time on several cores, any other gzip stream (one big member: gzip, pigz; concatenated members)
// through zlib's inflate.  The consumer (pc_gzstream_next) cuts the inflated bytes exactly where
// pc_readset_load_segment would cut the plain file -- a block holds the records that start before the first record
// start at or after `target_bytes` -- and parses it with all cores.
struct pc_gzstream {
    std::string path;
    std::thread producer;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Bytes> ready;
    size_t ready_bytes = 0;
    bool done = false, failed = false, stop = false;
    RawBuf pending;                      // inflated bytes not yet handed out (starts at a record start)
    bool eof = false;                    // the producer's last buffer has been taken
    int inflate_threads = 1;
    int64_t range_begin = 0, range_end = 0;   // compressed bytes [begin, end) of the file (member starts); end 0 = to the end of the file
    ~pc_gzstream()
    {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        if (producer.joinable()) producer.join();
    }
};

namespace {

constexpr size_t kGzQueueBytes = (size_t)512 << 20;     // inflated bytes the producer may run ahead
constexpr size_t kGzBuffer = (size_t)32 << 20;

// Members WITHOUT a size subfield -- `cat a.fastq.gz b.fastq.gz ...`, the usual way a run's thousands of small .gz files
// become one -- cannot be found by hopping, but they can be GUESSED: every member starts with 1f 8b 08 and a flag byte, and
// the four bytes before a true start are the previous member's ISIZE.  Worker threads inflate from the guessed starts ahead
// of the consumer (zlib checks each member's CRC and length itself); the consumer walks the file member by member and takes
// a guess's result only when a member really starts there -- a wrong guess (the magic inside compressed data) fails within a
// few hundred bytes or is simply never asked for.  A member larger than kSpecCap is left to the serial path (one core, streamed).
static const size_t kSpecCap = [] { const char *e = getenv("PC_GZ_SPEC_CAP_MB"); const long v = e ? atol(e) : 0; return (size_t)(v > 0 ? v : 256) << 20; }();

struct MemberSpeculator {
    const unsigned char *base;
    size_t size;
    struct Cand { size_t start; Bytes out; size_t end = 0; int state = 0; };   // 0 unclaimed, 1 running, 2 ok, 3 failed / too big
    std::deque<Cand> cands;              // ascending starts from `first_idx` on (consumed ones are dropped)
    size_t scan_pos = 0, consumed_pos = 0;
    int window;
    std::mutex mu;
    std::condition_variable cv;
    bool stop = false;
    std::vector<std::thread> workers;

    MemberSpeculator(const unsigned char *b, size_t n, size_t from, int threads) : base(b), size(n), scan_pos(from), consumed_pos(from), window(threads * 3)
    {
        for (int t = 0; t < threads; ++t) workers.emplace_back([this] { work(); });
    }
    ~MemberSpeculator()
    {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        for (auto &w : workers) w.join();
    }
    static bool magic_at(const unsigned char *p) { return p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && (p[3] & 0xE0) == 0; }
    // more guesses, while fewer than `window` are waiting (with mu held); a few megabytes per call -- ONE big member has no
    // guesses in it, and a scan of the whole file under the lock kept the consumer waiting at its first question
    // -> true when the budget, not the window or the end of the file, stopped it
    bool scan_more()
    {
        // (guesses the consumer has already passed are never claimed: they must not count, or a member whose data is dense
        // with the magic bytes fills the window with them and the scan never reaches the member the consumer asks for)
        size_t waiting = 0;
        for (const Cand &c : cands) if (c.state == 0 && c.start >= consumed_pos) ++waiting;
        const size_t budget_end = scan_pos + ((size_t)4 << 20);
        while (waiting < (size_t)window && scan_pos + 18 < size) {
            if (scan_pos >= budget_end) return true;
            const size_t stop = std::min(size - 18, budget_end);
            const unsigned char *q = (const unsigned char *)memchr(base + scan_pos, 0x1f, stop - scan_pos);
            if (!q) { scan_pos = stop; continue; }
            const size_t at = (size_t)(q - base);
            scan_pos = at + 1;
            if (!magic_at(q)) continue;
            cands.emplace_back();
            cands.back().start = at;
            ++waiting;
        }
        return false;
    }
    void work()
    {
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return;       // raw: header, CRC-32 and ISIZE are checked here (pc_gz.h)
        for (;;) {
            Cand *c = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    if (stop) { inflateEnd(&zs); return; }
                    const bool more = scan_more();
                    for (Cand &k : cands) if (k.state == 0 && k.start >= consumed_pos) { c = &k; break; }
                    if (c) { c->state = 1; break; }
                    if (more) { lk.unlock(); std::this_thread::yield(); lk.lock(); continue; }
                    cv.wait(lk);
                }
            }
            // (deque elements keep their addresses while others are pushed / popped at the ends)
            bool good = false;
            Bytes out;
            inflateReset(&zs);
            const size_t header = pcz::gzip_header_len(base + c->start, size - c->start);
            size_t at = c->start + header;
            zs.next_in = (Bytef *)(base + at); zs.avail_in = (uInt)std::min<size_t>(size - at, (size_t)1 << 30);
            const size_t in0 = zs.avail_in;
            size_t have = 0;
            uint32_t crc = 0;
            for (; header; ) {
                if (out.size() < have + ((size_t)64 << 10)) out.resize(std::max(out.size() * 2, have + ((size_t)512 << 10)));   // (most guesses die within a page)
                zs.next_out = (Bytef *)out.data() + have; zs.avail_out = (uInt)std::min<size_t>(out.size() - have, (size_t)1 << 30);
                const size_t room = zs.avail_out;
                const int r = inflate(&zs, Z_NO_FLUSH);
                crc = pcz::crc_update(crc, out.data() + have, room - zs.avail_out);
                have += room - zs.avail_out;
                if (r == Z_STREAM_END) {
                    const size_t trailer = at + (in0 - zs.avail_in);
                    good = trailer + pcz::kTrailer <= size && pcz::get32(base + trailer) == crc && pcz::get32(base + trailer + 4) == (uint32_t)have;
                    break;
                }
                if (r != Z_OK || have > kSpecCap || (zs.avail_in == 0 && zs.avail_out != 0)) break;
                { std::lock_guard<std::mutex> lk(mu); if (stop || c->start < consumed_pos) break; }      // nobody will ask for this one
            }
            std::lock_guard<std::mutex> lk(mu);
            if (good) { out.resize(have); c->out.swap(out); c->end = at + (in0 - zs.avail_in) + pcz::kTrailer; c->state = 2; }
            else c->state = 3;
            cv.notify_all();
        }
    }
    // Is the member that starts at `pos` small enough to be worth waiting for?  (The next plausible boundary -- a magic whose
    // preceding ISIZE fits the bytes in between -- lies within reach.)
    bool plausible_small_member(size_t pos) const
    {
        const size_t reach = std::min(size, pos + kSpecCap);
        for (size_t p = pos + 18; p + 4 <= reach; ) {
            const unsigned char *q = (const unsigned char *)memchr(base + p, 0x1f, reach - 4 - p);
            if (!q) break;
            p = (size_t)(q - base);
            if (magic_at(q)) {
                const size_t isize = pcz::get32(q - 4), gap = p - pos;
                if (isize <= kSpecCap && gap <= isize + isize / 8 + 128 && isize / 1100 <= gap) return true;   // (deflate neither expands nor shrinks beyond that)
            }
            ++p;
        }
        // the file's last member: its ISIZE are the last four bytes (before any zero padding)
        size_t e = size;
        while (e > pos + 18 && base[e - 1] == 0) --e;
        if (e <= reach && e >= pos + 18) { const size_t isize = pcz::get32(base + e - 4); return isize <= kSpecCap; }
        return false;
    }
    // The inflated member that starts at pos, if a worker has (or will soon have) it: *end = one past its last byte.
    bool take(size_t pos, Bytes &out, size_t *end)
    {
        std::unique_lock<std::mutex> lk(mu);
        consumed_pos = pos;
        // guesses behind the consumer are dead: unclaimed ones anywhere in the queue are marked so (elements a worker holds a
        // pointer to stay where they are: only the ends of a deque may go), finished ones leave from the front
        auto drop_stale = [&] {
            for (Cand &k : cands) { if (k.start >= pos) break; if (k.state == 0) k.state = 3; }
            while (!cands.empty() && cands.front().start < pos && cands.front().state != 1) cands.pop_front();
        };
        drop_stale();
        cv.notify_all();
        if (!plausible_small_member(pos)) return false;
        // never wait for ever: when nothing has moved for kPatience the caller inflates this member itself (serial zlib path)
        const auto t0 = std::chrono::steady_clock::now();
        const auto kPatience = std::chrono::seconds(20);
        for (;;) {
            while (scan_more() && scan_pos <= pos) {}
            Cand *c = nullptr;
            for (Cand &k : cands) { if (k.start == pos) { c = &k; break; } if (k.start > pos) break; }
            if (!c) {
                if (scan_pos > pos || scan_pos + 18 >= size) return false;          // scanned past it (or to the end): no member starts here
                drop_stale();
                if (std::chrono::steady_clock::now() - t0 > kPatience) return false;
                cv.wait_for(lk, std::chrono::milliseconds(1));
                continue;
            }
            if (c->state == 2) { out.swap(c->out); *end = c->end; c->state = 3; return true; }
            if (c->state == 3) return false;
            cv.notify_all();
            if (cv.wait_for(lk, std::chrono::milliseconds(200)) == std::cv_status::timeout &&
                std::chrono::steady_clock::now() - t0 > kPatience) {
                if (c->state == 0) c->state = 3;                                    // (a running worker notices consumed_pos moving on)
                return false;
            }
        }
    }
};

// ---- ONE big member at libdeflate's speed, still streamed ----------------------------------------------------------------
// libdeflate inflates 2-3 x faster than zlib but only whole buffers: no streaming interface.  It does, like any LZ77 decoder
// into a flat buffer, write its output strictly front to back (a match copy may run a few dozen bytes AHEAD of the position,
// never behind it).  So: the member is inflated by ONE libdeflate call on its own thread into fresh anonymous memory (zero
// pages until written), and this thread watches the output appear -- a probe every megabyte: non-zero bytes there mean the
// decoder has passed it -- and hands over what lies safely behind the front (256 KB: eight times the window the decoder may still
// read back into), block by block, its CRC-32 taken on the way and checked against the trailer at the end; pages handed
// over are given back to the kernel.  x86 keeps stores in order, so whatever lies behind a byte seen written has been
// written.  Output with 64 zero bytes at a probe only delays the hand-over until the call returns.
// The output size is not known (ISIZE is modulo 4 GiB): the room is `ratio` (12) times the compressed bytes, and the route is
// only taken when half the memory the process may still take holds 8 times; a member that needs more than the room is
// restarted by the caller through zlib, which discards what was handed over already.  PC_GZ_NO_ONESHOT=1 turns the route off; PC_GZ_ONESHOT_MIN_MB / PC_GZ_ONESHOT_RATIO tune it.
size_t memory_room()
{
    auto number_in = [](const char *path, const char *key) -> long long {
        FILE *f = fopen(path, "r");
        if (!f) return -1;
        char line[256];
        long long v = -1;
        while (fgets(line, sizeof line, f)) {
            if (!key) { if (line[0] >= '0' && line[0] <= '9') v = atoll(line); break; }
            if (!strncmp(line, key, strlen(key))) { v = atoll(line + strlen(key)); break; }
        }
        fclose(f);
        return v;
    };
    long long avail = number_in("/proc/meminfo", "MemAvailable:");
    avail = avail > 0 ? avail * 1024 : (long long)sysconf(_SC_AVPHYS_PAGES) * (long long)sysconf(_SC_PAGESIZE);
    long long cmax = number_in("/sys/fs/cgroup/memory.max", nullptr), ccur = number_in("/sys/fs/cgroup/memory.current", nullptr);     // (v2; "max" = no limit)
    if (cmax <= 0) { cmax = number_in("/sys/fs/cgroup/memory/memory.limit_in_bytes", nullptr); ccur = number_in("/sys/fs/cgroup/memory/memory.usage_in_bytes", nullptr); }
    if (cmax > 0 && ccur >= 0) avail = std::min(avail, std::max(0LL, cmax - ccur));
    return avail > 0 ? (size_t)avail : 0;
}

enum { kOneShotDone = 1, kOneShotNotTried = 0, kOneShotOutOfRoom = 2, kOneShotFailed = -1 };

// The member whose deflate data starts at base[*data_at]: -> kOneShotDone (*data_at = one past its trailer), kOneShotNotTried
// (nothing handed over: inflate it the ordinary way), kOneShotOutOfRoom (*handed bytes WERE handed over: inflate it the
// ordinary way and discard that many), kOneShotFailed (damaged, or the consumer is gone).
extern "C++" {
template <class Push>
int oneshot_member(const unsigned char *base, size_t size, size_t *data_at, Push &&push, size_t *handed)
{
    static const struct Knobs {
        bool off, verbose; size_t min_bytes; size_t ratio; size_t room_bytes;
        Knobs()
        {
            const char *o = getenv("PC_GZ_NO_ONESHOT"), *m = getenv("PC_GZ_ONESHOT_MIN_MB"), *r = getenv("PC_GZ_ONESHOT_RATIO");
            const char *v = getenv("PC_GZ_VERBOSE"), *rm = getenv("PC_GZ_ONESHOT_ROOM_KB");       // (tests: a room too small on purpose)
            verbose = v && *v && *v != '0';
            room_bytes = (size_t)(rm && atol(rm) > 0 ? atol(rm) : 0) << 10;
            off = o && *o && *o != '0';
            min_bytes = (size_t)(m && atol(m) >= 0 ? atol(m) : 32) << 20;
            ratio = (size_t)(r && atol(r) > 0 ? atol(r) : 12);
        }
    } knobs;
    const pcz::LibDeflate &ld = pcz::libdeflate();
    *handed = 0;
    const size_t at = *data_at;
#if !defined(__x86_64__) && !defined(__i386__)
    // the hand-over below reads another thread's output through nothing but the stores' order: sound on x86 (stores are not
    // reordered with older stores), not on weakly ordered hosts -- those inflate the member the ordinary way
    return kOneShotNotTried;
#endif
    if (knobs.off || !ld.ok || !ld.deflate_decompress_ex || at + pcz::kTrailer >= size) return kOneShotNotTried;
    const size_t in_n = size - at - pcz::kTrailer;            // at most this much deflate data (the call stops at the end of the stream)
    if (in_n < knobs.min_bytes) return kOneShotNotTried;
    size_t room = std::min(in_n * knobs.ratio + ((size_t)64 << 20), memory_room() / 2) & ~(size_t)4095;
    // (FASTQ inflates 3-7 x: with less than 8 x within reach the member might outgrow the room after gigabytes were handed over,
    // and zlib would inflate all of it again -- memory that tight streams through zlib from the start)
    if (room < in_n * std::min<size_t>(8, knobs.ratio)) return kOneShotNotTried;
    if (knobs.room_bytes) room = std::max<size_t>(knobs.room_bytes, 8192) & ~(size_t)4095;
    // Peak memory of this route: the decoder cannot be paused (ONE libdeflate call), so while the consumer is slower than it
    // (push() blocks on the 512 MB queue) the inflated member piles up in the mapping -- pages are returned only once handed
    // over.  The room is therefore the bound: at most half of what the process could still take when the member began
    // (memory_room: MemAvailable and the cgroup's limit), PC_GZ_ONESHOT_MAX_MB caps it further (several processes on one
    // box: each sees the same free memory), and a member that outgrows it is restarted through zlib's streaming inflate.
    {
        static const size_t cap = [] { const char *e = getenv("PC_GZ_ONESHOT_MAX_MB"); const long v = e ? atol(e) : 0; return v > 0 ? (size_t)v << 20 : (size_t)0; }();
        if (cap && room > cap) {
            if (cap < in_n * std::min<size_t>(8, knobs.ratio)) return kOneShotNotTried;
            room = cap & ~(size_t)4095;
        }
    }
    void *mem = mmap(nullptr, room, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (mem == MAP_FAILED) return kOneShotNotTried;
    void *dec = ld.alloc_decompressor();
    if (!dec) { munmap(mem, room); return kOneShotNotTried; }
    unsigned char *out = (unsigned char *)mem;
    std::atomic<int> finished{0};
    size_t used_in = 0, made = 0;
    int rc = 1;
    std::thread decoder([&] {
        rc = ld.deflate_decompress_ex(dec, base + at, in_n, out, room, &used_in, &made);
        finished.store(1, std::memory_order_release);
    });
    constexpr size_t kStride = (size_t)1 << 20, kBehind = (size_t)256 << 10;
    auto written_at = [&](size_t p) {
        const volatile unsigned char *q = out + p;
        for (int k = 0; k < 64; ++k) if (q[k]) return true;
        return false;
    };
    size_t released = 0, dropped = 0, front = 0;          // front: a multiple of kStride whose probe has been seen written
    uint32_t crc = 0;
    bool consumer_gone = false;
    auto release_to = [&](size_t upto) {
        std::atomic_thread_fence(std::memory_order_acquire);
        while (released < upto && !consumer_gone) {
            const size_t n = std::min(kGzBuffer, upto - released);
            Bytes b(n);
            memcpy(b.data(), out + released, n);
            crc = pcz::crc_update(crc, b.data(), n);
            released += n;
            if (!push(std::move(b))) consumer_gone = true;
            const size_t keep = released & ~(size_t)4095;
            if (keep > dropped) { madvise(out + dropped, keep - dropped, MADV_DONTNEED); dropped = keep; }
        }
    };
    while (!finished.load(std::memory_order_acquire)) {
        while (front + kStride + 64 <= room && written_at(front + kStride)) front += kStride;
        if (!consumer_gone && front > kBehind && front - kBehind > released + ((size_t)4 << 20)) release_to(front - kBehind);
        else std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    decoder.join();
    ld.free_decompressor(dec);
    int result;
    if (consumer_gone) result = kOneShotFailed;
    else if (rc == 0) {
        release_to(made);
        const size_t trailer = at + used_in;
        const bool good = !consumer_gone && trailer + pcz::kTrailer <= size && pcz::get32(base + trailer) == crc && pcz::get32(base + trailer + 4) == (uint32_t)made;
        if (good) *data_at = trailer + pcz::kTrailer;
        result = good ? kOneShotDone : kOneShotFailed;
    } else if (rc == 3) {
        result = released ? kOneShotOutOfRoom : kOneShotNotTried;
    } else {
        result = released ? kOneShotFailed : kOneShotNotTried;          // (zlib will say the same about a damaged stream)
    }
    *handed = released;
    munmap(mem, room);
    if (knobs.verbose) fprintf(stderr, "pc_gz: one-shot member at %zu: rc %d, %zu -> %zu bytes, %zu handed over, result %d\n", at, rc, used_in, made, released, result);
    return result;
}
}  // extern "C++"

void gz_produce(pc_gzstream *s)
{
    auto push = [&](Bytes &&v) -> bool {
        std::unique_lock<std::mutex> lk(s->mu);
        s->cv.wait(lk, [&] { return s->stop || s->ready_bytes < kGzQueueBytes; });
        if (s->stop) return false;
        s->ready_bytes += v.size();
        s->ready.push_back(std::move(v));
        lk.unlock();
        s->cv.notify_all();
        return true;
    };
    auto finish = [&](bool ok) {
        { std::lock_guard<std::mutex> lk(s->mu); s->done = true; s->failed = !ok; }
        s->cv.notify_all();
    };
    const int fd = open(s->path.c_str(), O_RDONLY);
    if (fd < 0) { finish(false); return; }
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size <= 0) { close(fd); finish(false); return; }
    const size_t map_size = (size_t)st.st_size;
    // (a byte range of the file -- pc_gzstream_open_range: the members between two member starts, one rank's share of a
    // sharded run -- is the same stream with its beginning and end moved)
    const size_t size = (s->range_end > 0 && (size_t)s->range_end < map_size) ? (size_t)s->range_end : map_size;
    void *m = mmap(nullptr, map_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) { finish(false); return; }
    madvise(m, map_size, MADV_SEQUENTIAL);
    const unsigned char *base = (const unsigned char *)m;
    bool ok = true;
    size_t at = (size_t)std::max<int64_t>(0, std::min<int64_t>(s->range_begin, (int64_t)size));
    // ---- members that carry their size: batches of about kGzBuffer inflated bytes, several threads -----------------
    while (ok && at < size) {
        struct Member { size_t in, in_n, out, out_n; uint32_t crc; };
        std::vector<Member> mem;
        size_t total = 0, p = at;
        while (p < size && total < kGzBuffer) {
            size_t payload = 0;
            const size_t n = pcz::sized_member(base + p, size - p, &payload);
            if (!n) break;
            const size_t isize = pcz::get32(base + p + n - 4);
            mem.push_back({p + payload, n - payload - pcz::kTrailer, total, isize, pcz::get32(base + p + n - 8)});
            total += isize;
            p += n;
        }
        if (mem.empty()) break;                           // an ordinary gzip member from here on
        Bytes buf(total);
        const int T = std::max(1, std::min<int>(s->inflate_threads, (int)(mem.size() / 16 + 1)));
        std::atomic<size_t> next{0};
        std::atomic<bool> good{true};
        auto work = [&]() {
            pcz::Inflater inf;
            for (;;) {
                const size_t i0 = next.fetch_add(16);
                if (i0 >= mem.size() || !good.load()) return;
                for (size_t i = i0; i < std::min(mem.size(), i0 + 16); ++i)
                    if (!inf.raw(base + mem[i].in, mem[i].in_n, buf.data() + mem[i].out, mem[i].out_n, mem[i].crc)) { good.store(false); return; }
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back(work);
        work();
        for (auto &x : th) x.join();
        if (!good.load()) { ok = false; break; }
        at = p;
        if (total && !push(std::move(buf))) { munmap(m, map_size); finish(false); return; }
    }
    // ---- the rest (all of an ordinary .gz file): zlib's inflate, member after member -------------------------------
    if (ok && at < size) {
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) ok = false;    // raw: header, CRC-32 and ISIZE are checked here (pc_gz.h)
        Bytes buf;
        bool ended = false;                               // the last member has ended and nothing follows it
        bool in_member = false;
        uint32_t crc = 0, isize = 0;
        static const bool no_spec = [] { const char *e = getenv("PC_GZ_NO_SPECULATION"); return e && *e && *e != '0'; }();
        std::unique_ptr<MemberSpeculator> spec;
        if (!no_spec && s->inflate_threads > 1 && size - at > ((size_t)1 << 20)) spec.reset(new MemberSpeculator(base, size, at, s->inflate_threads));
        // members that workers have inflated ahead (see MemberSpeculator): taken whole, one after the other, for as long as
        // a member starts where the last one ended
        auto take_ahead = [&]() -> bool {
            while (spec && ok && !ended) {
                Bytes whole;
                size_t end = 0;
                if (!spec->take(at, whole, &end)) return true;
                at = end;
                while (at < size && base[at] == 0) ++at;
                if (at >= size) ended = true;
                if (!whole.empty() && !push(std::move(whole))) return false;
            }
            return true;
        };
        if (!take_ahead()) { inflateEnd(&zs); spec.reset(); munmap(m, map_size); finish(false); return; }
        size_t discard = 0;                               // inflated bytes of the current member that were handed over already
        while (ok && !ended) {
            if (!in_member && !discard) {
                // a big member the workers did not take: one libdeflate call, watched (oneshot_member)
                const size_t header = pcz::gzip_header_len(base + at, size - at);
                size_t data_at = at + header, handed = 0;
                const int one = header ? oneshot_member(base, size, &data_at, push, &handed) : kOneShotNotTried;
                if (one == kOneShotFailed) { if (s->stop) { inflateEnd(&zs); spec.reset(); munmap(m, map_size); finish(false); return; } ok = false; break; }
                if (one == kOneShotOutOfRoom) discard = handed;
                if (one == kOneShotDone) {
                    at = data_at;
                    while (at < size && base[at] == 0) ++at;
                    if (at >= size) { ended = true; break; }
                    if (!take_ahead()) { inflateEnd(&zs); spec.reset(); munmap(m, map_size); finish(false); return; }
                    continue;
                }
            }
            buf.resize(kGzBuffer);
            zs.next_out = (Bytef *)buf.data(); zs.avail_out = (uInt)buf.size();
            while (zs.avail_out) {
                if (!in_member) {
                    const size_t header = pcz::gzip_header_len(base + at, size - at);
                    if (!header || inflateReset(&zs) != Z_OK) { ok = false; break; }      // (anything but a member after a member: an error, as for Python's gzip)
                    at += header;
                    in_member = true; crc = 0; isize = 0;
                }
                const size_t take = std::min<size_t>(size - at, (size_t)1 << 30);
                zs.next_in = (Bytef *)(base + at); zs.avail_in = (uInt)take;
                const Bytef *out0 = zs.next_out;
                const int r = inflate(&zs, Z_NO_FLUSH);
                at += take - zs.avail_in;
                crc = pcz::crc_update(crc, out0, (size_t)(zs.next_out - out0));
                isize += (uint32_t)(zs.next_out - out0);
                if (r == Z_STREAM_END) {
                    if (at + pcz::kTrailer > size || pcz::get32(base + at) != crc || pcz::get32(base + at + 4) != isize) { ok = false; break; }
                    at += pcz::kTrailer;
                    in_member = false;
                    // another member may follow (zeros after the last member are padding, as gzip treats them)
                    while (at < size && base[at] == 0) ++at;
                    if (at >= size) { ended = true; break; }
                    if (spec) break;                      // (hand what there is over, then see whether the next members were inflated ahead)
                    continue;
                }
                if (r == Z_OK) continue;
                ok = false;                               // Z_BUF_ERROR with room left: the file ends inside a member; or damage
                break;
            }
            if (!ok) break;
            buf.resize(buf.size() - zs.avail_out);
            if (discard) {                                // (the one-shot route ran out of room after handing this much over)
                const size_t drop = std::min(discard, buf.size());
                buf.erase(buf.begin(), buf.begin() + (ptrdiff_t)drop);
                discard -= drop;
            }
            if (!in_member) discard = 0;
            if (!buf.empty() && !push(std::move(buf))) { inflateEnd(&zs); spec.reset(); munmap(m, map_size); finish(false); return; }
            buf = Bytes();
            if (spec && ok && !ended && !in_member && !take_ahead()) { inflateEnd(&zs); spec.reset(); munmap(m, map_size); finish(false); return; }
        }
        spec.reset();
        inflateEnd(&zs);
    }
    munmap(m, map_size);
    finish(ok);
}

extern "C++" bool inflate_whole_gzip(const char *path, RawBuf &out)         // (declared above, outside the extern "C" block)
{
    pc_gzstream s;                                        // (its destructor stops and joins the producer)
    s.path = path;
    s.inflate_threads = std::max(1, usable_threads());
    s.producer = std::thread(gz_produce, &s);
    out.resize(0);
    for (;;) {
        std::unique_lock<std::mutex> lk(s.mu);
        s.cv.wait(lk, [&] { return !s.ready.empty() || s.done; });
        if (s.ready.empty()) return !s.failed;
        Bytes v = std::move(s.ready.front());
        s.ready.pop_front();
        s.ready_bytes -= v.size();
        lk.unlock();
        s.cv.notify_all();
        out.append(v.data(), v.data() + v.size());
    }
}

}  // namespace

// -> PC_ERR_UNSUPPORTED_SCORES ("not streamable") when the file is not gzip
int pc_gzstream_open(const char *path, pc_gzstream **out)
{
    if (!path || !out) return PC_ERR_BAD_ARG;
    *out = nullptr;
    FILE *f = fopen(path, "rb");
    if (!f) return PC_ERR_BAD_ARG;
    unsigned char magic[3] = {0, 0, 0};
    const size_t got = fread(magic, 1, 3, f);
    fclose(f);
    if (got < 3 || magic[0] != 0x1f || magic[1] != 0x8b || magic[2] != 8) return PC_ERR_UNSUPPORTED_SCORES;
    pc_gzstream *s = new pc_gzstream();
    s->path = path;
    s->inflate_threads = std::max(1, usable_threads() / 2);
    s->producer = std::thread(gz_produce, s);
    *out = s;
    return PC_OK;
}

// The same stream over the members that lie in [begin, end) of the file's COMPRESSED bytes (both member starts, as
// pc_gz_member_start finds them; end <= 0: to the end of the file): one rank's share of a gzip file that is not made of
// sized members -- `cat *.fastq.gz`, the way a run's many small files usually become one.
int pc_gzstream_open_range(const char *path, int64_t begin, int64_t end, pc_gzstream **out)
{
    if (!path || !out || begin < 0) return PC_ERR_BAD_ARG;
    *out = nullptr;
    FILE *f = fopen(path, "rb");
    if (!f) return PC_ERR_BAD_ARG;
    unsigned char magic[3] = {0, 0, 0};
    const bool at_member = fseeko(f, (off_t)begin, SEEK_SET) == 0 && fread(magic, 1, 3, f) == 3 && magic[0] == 0x1f && magic[1] == 0x8b && magic[2] == 8;
    fclose(f);
    if (!at_member) return PC_ERR_UNSUPPORTED_SCORES;
    pc_gzstream *s = new pc_gzstream();
    s->path = path;
    s->range_begin = begin; s->range_end = end > 0 ? end : 0;
    s->inflate_threads = std::max(1, usable_threads() / 2);
    s->producer = std::thread(gz_produce, s);
    *out = s;
    return PC_OK;
}

// The first gzip member that starts at or after byte `pos` of the file (the file's size when there is none): a candidate is
// where the member magic stands (1f 8b 08 + a flag byte without reserved bits); it IS a member start when the deflate stream
// behind it inflates to its end and the trailer's CRC-32 and ISIZE agree with what came out (a candidate inside compressed
// data fails within a few hundred bytes; passing the check by accident takes a 64-bit coincidence).  Lets the ranks of a
// sharded run cut an ordinary multi-member gzip file at member boundaries without anyone inflating all of it.
int pc_gz_member_start(const char *path, int64_t pos, int64_t *member_start)
{
    if (!path || !member_start || pos < 0) return PC_ERR_BAD_ARG;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return PC_ERR_BAD_ARG;
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size <= 0) { close(fd); return PC_ERR_UNSUPPORTED_SCORES; }
    const size_t size = (size_t)st.st_size;
    if ((size_t)pos >= size) { close(fd); *member_start = (int64_t)size; return PC_OK; }
    void *m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return PC_ERR_UNSUPPORTED_SCORES;
    const unsigned char *base = (const unsigned char *)m;
    int rc = PC_OK;
    if (!(base[0] == 0x1f && base[1] == 0x8b && base[2] == 8)) rc = PC_ERR_UNSUPPORTED_SCORES;
    int64_t found = (int64_t)size;
    if (rc == PC_OK && pos == 0) found = 0;
    if (rc == PC_OK && pos > 0) {
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) rc = PC_ERR_BAD_ARG;
        std::vector<unsigned char> outb((size_t)1 << 20);
        for (size_t p = (size_t)pos; rc == PC_OK && p + 18 < size; ) {
            const unsigned char *q = (const unsigned char *)memchr(base + p, 0x1f, size - 18 - p);
            if (!q) break;
            p = (size_t)(q - base);
            if (!(q[1] == 0x8b && q[2] == 8 && (q[3] & 0xE0) == 0)) { ++p; continue; }
            const size_t header = pcz::gzip_header_len(q, size - p);
            bool good = false;
            if (header && inflateReset(&zs) == Z_OK) {
                size_t at = p + header;
                uint32_t crc = 0;
                uint64_t have = 0;
                for (;;) {
                    zs.next_in = (Bytef *)(base + at); zs.avail_in = (uInt)std::min<size_t>(size - at, (size_t)1 << 30);
                    const size_t in0 = zs.avail_in;
                    zs.next_out = outb.data(); zs.avail_out = (uInt)outb.size();
                    const int r = inflate(&zs, Z_NO_FLUSH);
                    const size_t made = outb.size() - zs.avail_out;
                    crc = pcz::crc_update(crc, outb.data(), made);
                    have += made;
                    at += in0 - zs.avail_in;
                    if (r == Z_STREAM_END) {
                        good = at + pcz::kTrailer <= size && pcz::get32(base + at) == crc && pcz::get32(base + at + 4) == (uint32_t)have;
                        break;
                    }
                    if (r != Z_OK || (made == 0 && in0 == zs.avail_in)) break;
                }
            }
            if (good) { found = (int64_t)p; break; }
            ++p;
        }
        inflateEnd(&zs);
    }
    if (rc == PC_OK) *member_start = found;
    munmap(m, size);
    return rc;
}

// The next block: the records that start before the first record start at or after target_bytes of the bytes not yet
// handed out, and at least min_reads of them (phase A's check reads must sit in the first block) unless the file ends
// first.  *out = null and *eof = 1 after the last block.  PC_ERR_UNSUPPORTED_SCORES: not a regular 4-line FASTQ (or a
// damaged gzip stream): the caller loads the whole file with pc_readset_load, which reproduces the reference's behaviour
// and messages for such inputs.
int pc_gzstream_next(pc_gzstream *s, int64_t target_bytes, int64_t min_reads, pc_readset **out, int *eof)
{
    if (!s || !out || !eof || target_bytes <= 0) return PC_ERR_BAD_ARG;
    *out = nullptr; *eof = 0;
    size_t target = (size_t)target_bytes;
    for (;;) {                      // (a FASTA block that would end in a header without a name is cut again, further on)
        const char *cut = nullptr;
        bool fasta = false;
        for (;;) {
            // enough bytes for a cut after `target`?
            const char *base = s->pending.data(), *end = base + s->pending.size();
            fasta = s->pending.size() && base[0] == '>';
            if (s->pending.size() && base[0] != '@' && !fasta) return PC_ERR_UNSUPPORTED_SCORES;
            cut = nullptr;
            if (s->pending.size() > target) {
                cut = fasta ? find_fasta_record_start(base + target, base, end) : find_record_start(base + target, base, end);
                if (cut && min_reads > 0) {
                    int64_t recs = 0;
                    if (fasta) {
                        for (const char *q = base; q < cut; ) { if (*q == '>') ++recs; const char *nl = (const char *)memchr(q, '\n', (size_t)(cut - q)); if (!nl) break; q = nl + 1; }
                    } else {
                        int64_t lines = 0;
                        for (const char *q = base; q < cut; ) { const char *nl = (const char *)memchr(q, '\n', (size_t)(cut - q)); if (!nl) break; ++lines; q = nl + 1; }
                        recs = lines / 4;
                    }
                    if (recs < min_reads) { target = std::max(target * 2, (size_t)(cut - base) + 1); cut = nullptr; continue; }
                }
            }
            if (cut) break;
            if (s->eof) { cut = end; break; }
            // take what the producer has
            std::unique_lock<std::mutex> lk(s->mu);
            s->cv.wait(lk, [&] { return !s->ready.empty() || s->done; });
            if (s->ready.empty()) {
                if (s->failed) return PC_ERR_UNSUPPORTED_SCORES;
                s->eof = true;
                continue;
            }
            Bytes v = std::move(s->ready.front());
            s->ready.pop_front();
            s->ready_bytes -= v.size();
            lk.unlock();
            s->cv.notify_all();
            s->pending.append(v.data(), v.data() + v.size());
        }
        const char *base = s->pending.data(), *end = base + s->pending.size();
        if (cut == base) { *eof = 1; return PC_OK; }
        pc_readset *rs = new pc_readset();
        rs->fastq = !fasta;
        if (fasta) {
            const bool last = s->eof && cut == end;
            if (!parse_fasta_range(rs, base, cut, usable_threads(), last)) {       // its last header has no name: the bases go on
                delete rs;
                target = (size_t)(cut - base) + 1;
                continue;
            }
        } else if (!parse_fastq_range(rs, base, cut, usable_threads())) { delete rs; return PC_ERR_UNSUPPORTED_SCORES; }
        rs->file_index.resize(rs->off.size(), 0);
        rs->arena.fill(64, 'N');
        const size_t rest = (size_t)(end - cut);
        if (rest) memmove(s->pending.data(), cut, rest);
        s->pending.resize(rest);
        *out = rs;
        return PC_OK;
    }
}

void pc_gzstream_close(pc_gzstream *s) { delete s; }

void pc_readset_free(pc_readset *rs) { delete rs; }
const char *pc_readset_error(const pc_readset *rs) { return rs ? rs->error.c_str() : "null readset"; }
int64_t pc_readset_count(const pc_readset *rs) { return rs ? (int64_t)rs->off.size() : 0; }
int pc_readset_is_fastq(const pc_readset *rs) { return rs && rs->fastq ? 1 : 0; }
const char *pc_readset_arena(const pc_readset *rs, int64_t *bytes)
{
    if (!rs) return nullptr;
    if (bytes) *bytes = (int64_t)rs->arena.size();
    return rs->arena.data();
}
const int64_t *pc_readset_offsets(const pc_readset *rs) { return rs ? rs->off.data() : nullptr; }
const int32_t *pc_readset_lengths(const pc_readset *rs) { return rs ? rs->len.data() : nullptr; }
const char *pc_readset_name(const pc_readset *rs, int64_t i)
{
    return (rs && i >= 0 && i < (int64_t)rs->name_off.size()) ? rs->name_of((size_t)i) : nullptr;
}
// " " + text[k] behind the stored header of read read[k]: every writer and pc_readset_name read the header from the name
// arena, which is rebuilt once, in read order.  Everything is checked before anything changes.
int pc_readset_annotate(pc_readset *rs, int64_t n, const int64_t *read, const char *const *text)
{
    if (!rs || n < 0 || (n > 0 && (!read || !text))) return PC_ERR_BAD_ARG;
    const int64_t R = (int64_t)rs->name_off.size();
    size_t extra = 0;
    for (int64_t k = 0; k < n; ++k) {
        if (read[k] < 0 || read[k] >= R || !text[k] || !text[k][0]) return PC_ERR_BAD_ARG;
        if (strpbrk(text[k], "\n\r")) return PC_ERR_BAD_ARG;
        extra += 1 + strlen(text[k]);
    }
    if (n == 0) return PC_OK;
    // the texts of a read, in the order given (a stable counting sort by read)
    std::vector<int64_t> first((size_t)R + 1, 0), order((size_t)n);
    for (int64_t k = 0; k < n; ++k) ++first[(size_t)read[k] + 1];
    for (int64_t r = 0; r < R; ++r) first[(size_t)r + 1] += first[(size_t)r];
    {
        std::vector<int64_t> next(first.begin(), first.end() - 1);
        for (int64_t k = 0; k < n; ++k) order[(size_t)next[(size_t)read[k]]++] = k;
    }
    std::vector<char> fresh;
    fresh.reserve(rs->name_arena.size() + extra);
    std::vector<int64_t> fresh_off((size_t)R);
    for (int64_t r = 0; r < R; ++r) {
        fresh_off[(size_t)r] = (int64_t)fresh.size();
        const char *name = rs->name_of((size_t)r);
        fresh.insert(fresh.end(), name, name + strlen(name));
        for (int64_t t = first[(size_t)r]; t < first[(size_t)r + 1]; ++t) {
            const char *s = text[(size_t)order[(size_t)t]];
            fresh.push_back(' ');
            fresh.insert(fresh.end(), s, s + strlen(s));
        }
        fresh.push_back('\0');
    }
    rs->name_arena.resize(fresh.size());
    memcpy(rs->name_arena.data(), fresh.data(), fresh.size());
    rs->name_off.swap(fresh_off);
    return PC_OK;
}
const char *pc_readset_quals(const pc_readset *rs, int64_t i)
{
    return (rs && rs->fastq && i >= 0 && i < (int64_t)rs->qual_off.size()) ? rs->qual_of((size_t)i) : nullptr;
}
int pc_readset_is_rna(const pc_readset *rs, int64_t i)
{
    return (rs && i >= 0 && i < (int64_t)rs->rna.size()) ? rs->rna[(size_t)i] : 0;
}
const int32_t *pc_readset_file_index(const pc_readset *rs) { return rs ? rs->file_index.data() : nullptr; }

// ---- 2-bit packing of the read bases for the trip over PCIe (include/porechop_amd.h, pc_pack_reads) ---------------
// Codes are SeqAn's Dna ordinal values (seqan/basic/alphabet_residue_tabs.h:113-140: A 0, C 1, G 2, T/U 3, either case);
// every other byte is an exception (Dna5 'N' for the alignment) whose POSITION is listed.  Threads take spans that are
// multiples of 64 bases, so no two threads share a byte of the plane; the exception lists of the spans are concatenated
// in span order, which leaves them sorted.
int pc_pack_reads(const char *arena, int64_t nbases, uint8_t *packed, int64_t *exc_pos, int64_t exc_cap, int64_t *nexc)
{
    if (nbases < 0 || (nbases && (!arena || !packed)) || !nexc) return PC_ERR_BAD_ARG;
    static const struct Tab { uint8_t t[256]; Tab() { memset(t, 4, sizeof t); t['A'] = t['a'] = 0; t['C'] = t['c'] = 1; t['G'] = t['g'] = 2;
                                                      t['T'] = t['t'] = t['U'] = t['u'] = 3; } } tab;
    const int64_t blocks = (nbases + 63) / 64;
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(usable_threads(), blocks / 4096 + 1));
    std::vector<std::vector<int64_t>> exc((size_t)T);
    auto work = [&](int t) {
        const int64_t b0 = blocks * t / T * 64, b1 = std::min<int64_t>(nbases, blocks * (t + 1) / T * 64);
        const unsigned char *src = (const unsigned char *)arena;
        std::vector<int64_t> &mine = exc[(size_t)t];
        int64_t i = b0;
        for (; i + 4 <= b1; i += 4) {
            const unsigned a = tab.t[src[i]], b = tab.t[src[i + 1]], c = tab.t[src[i + 2]], d = tab.t[src[i + 3]];
            if ((a | b | c | d) & 4u) {
                if (a & 4u) mine.push_back(i);
                if (b & 4u) mine.push_back(i + 1);
                if (c & 4u) mine.push_back(i + 2);
                if (d & 4u) mine.push_back(i + 3);
            }
            packed[i >> 2] = (uint8_t)((a & 3u) | (b & 3u) << 2 | (c & 3u) << 4 | (d & 3u) << 6);
        }
        if (i < b1) {                                   // the last, partial byte of the plane (only the last span has one)
            unsigned v = 0;
            for (int k = 0; i + k < b1; ++k) {
                const unsigned a = tab.t[src[i + k]];
                if (a & 4u) mine.push_back(i + k);
                v |= (a & 3u) << (2 * k);
            }
            packed[i >> 2] = (uint8_t)v;
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
    int64_t total = 0;
    for (auto &v : exc) total += (int64_t)v.size();
    *nexc = total;
    if (total > exc_cap || (total && !exc_pos)) return PC_ERR_BAD_ARG;        // *nexc says how many entries are needed
    int64_t at = 0;
    for (auto &v : exc) { if (!v.empty()) memcpy(exc_pos + at, v.data(), v.size() * 8); at += (int64_t)v.size(); }
    return PC_OK;
}

static int write_pieces(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                        const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                        const char *const *file_paths, int fastq, int64_t *bytes_written, int64_t *file_pos,
                        int shared = 0, int64_t *sizes_only = nullptr, pc_gzimage *image = nullptr, int gz_level = 6);

void pc_io_set_thread_limit(int nthreads) { t_thread_limit = nthreads > 0 ? (nthreads > 64 ? 64 : nthreads) : 0; }

int pc_readset_write(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                     const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                     const char *const *file_paths, int fastq, int64_t *bytes_written)
{
    return write_pieces(rs, npieces, piece_read, piece_start, piece_len, piece_number, piece_file, nfiles, file_paths, fastq,
                        bytes_written, nullptr);
}

// The same, block after block of a streamed input: file_pos[f] is where file f continues (0: create / truncate it now),
// updated to where it ends after this call.
int pc_readset_write_at(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                        const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                        const char *const *file_paths, int fastq, int64_t *file_pos)
{
    if (!file_pos) return PC_ERR_BAD_ARG;
    return write_pieces(rs, npieces, piece_read, piece_start, piece_len, piece_number, piece_file, nfiles, file_paths, fastq,
                        nullptr, file_pos);
}

// The write of one rank of a sharded run: like pc_readset_write_at, but the files are SHARED with other processes writing
// disjoint spans -- they are opened without truncation whatever the position (the caller creates / truncates them once,
// before any rank writes).
int pc_readset_write_shared(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                            const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                            const char *const *file_paths, int fastq, int64_t *file_pos)
{
    if (!file_pos) return PC_ERR_BAD_ARG;
    return write_pieces(rs, npieces, piece_read, piece_start, piece_len, piece_number, piece_file, nfiles, file_paths, fastq,
                        nullptr, file_pos, 1);
}

// How many bytes pc_readset_write would put into each file (bytes_per_file[nfiles]); nothing is written or created.
int pc_readset_write_sizes(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                           const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                           int fastq, int64_t *bytes_per_file)
{
    if (!bytes_per_file || nfiles < 0) return PC_ERR_BAD_ARG;
    for (int f = 0; f < nfiles; ++f) bytes_per_file[f] = 0;
    std::vector<const char *> dummy((size_t)std::max(nfiles, 1), "");
    return write_pieces(rs, npieces, piece_read, piece_start, piece_len, piece_number, piece_file, nfiles, dummy.data(), fastq,
                        nullptr, nullptr, 0, bytes_per_file);
}

// The same pieces, formatted and DEFLATED by all cores into memory (pc_gz.h: independent members that carry their size):
// what the reference gets from `pigz -p <threads>` over its temporary file (porechop.py:640-651,685-729).  Nothing is
// opened or written; pc_gzimage_write puts the image of every file where the caller says (a streamed run appends block
// after block, the ranks of a sharded run exchange pc_gzimage_sizes first), pc_gz_finish ends a file.
int pc_readset_compress(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                        const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                        int fastq, int level, pc_gzimage **out)
{
    if (!out || nfiles < 0) return PC_ERR_BAD_ARG;
    pc_gzimage *img = new pc_gzimage();
    img->parts.resize((size_t)nfiles);
    img->plain.assign((size_t)nfiles, 0);
    *out = img;
    std::vector<const char *> dummy((size_t)std::max(nfiles, 1), "");
    return write_pieces(rs, npieces, piece_read, piece_start, piece_len, piece_number, piece_file, nfiles, dummy.data(), fastq,
                        nullptr, nullptr, 0, nullptr, img, pcz::default_level(level));
}

int pc_gzimage_sizes(const pc_gzimage *img, int nfiles, int64_t *compressed_bytes, int64_t *plain_bytes)
{
    if (!img || nfiles != (int)img->parts.size() || !compressed_bytes) return PC_ERR_BAD_ARG;
    for (int f = 0; f < nfiles; ++f) {
        compressed_bytes[f] = img->bytes((size_t)f);
        if (plain_bytes) plain_bytes[f] = img->plain[(size_t)f];
    }
    return PC_OK;
}

// file_pos[f]: where file f's image goes (0 and not shared: the file is created / truncated), updated to its end.  Files
// whose image is empty are not touched.
int pc_gzimage_write(const pc_gzimage *img, int nfiles, const char *const *file_paths, int64_t *file_pos, int shared)
{
    if (!img || nfiles != (int)img->parts.size() || (nfiles && (!file_paths || !file_pos))) return PC_ERR_BAD_ARG;
    int rc = PC_OK;
    for (int f = 0; f < nfiles && rc == PC_OK; ++f) {
        const auto &parts = img->parts[(size_t)f];
        if (img->bytes((size_t)f) == 0) continue;
        const int64_t base = file_pos[f];
        const int fd = open(file_paths[f], shared ? (O_RDWR | O_CREAT) : (base ? O_RDWR : (O_RDWR | O_CREAT | O_TRUNC)), 0666);
        if (fd < 0) return PC_ERR_BAD_ARG;
        int64_t at = base;
        for (const auto &v : parts) {
            size_t done = 0;
            while (done < v.size()) {
                const ssize_t w = pwrite(fd, v.data() + done, v.size() - done, (off_t)(at + (int64_t)done));
                if (w <= 0) { rc = PC_ERR_BAD_ARG; break; }
                done += (size_t)w;
            }
            if (rc != PC_OK) break;
            at += (int64_t)v.size();
        }
        if (close(fd) != 0) rc = PC_ERR_BAD_ARG;
        file_pos[f] = at;
    }
    return rc;
}

void pc_gzimage_free(pc_gzimage *img) { delete img; }

// The last member of a file of sized members: the empty one (28 bytes).  Creates the file when there is none (the
// reference always leaves an output file behind: the gzip of nothing).
int pc_gz_finish(const char *path)
{
    if (!path) return PC_ERR_BAD_ARG;
    const int fd = open(path, O_WRONLY | O_CREAT | O_APPEND, 0666);
    if (fd < 0) return PC_ERR_BAD_ARG;
    const bool ok = write(fd, pcz::kEofBlock, sizeof pcz::kEofBlock) == (ssize_t)sizeof pcz::kEofBlock;
    return (close(fd) == 0 && ok) ? PC_OK : PC_ERR_BAD_ARG;
}

// A whole file through the same compressor, all cores: src -> dst.  single_member = 0: sized members (pc_gz.h);
// 1: ONE gzip member the way pigz makes it -- every block deflated on its own, ended at a byte boundary by a sync
// flush, the blocks concatenated and their CRCs combined -- i.e. input nobody can inflate in parallel (bench / tests:
// the reader's streamed route for ordinary .gz files).
int pc_gzip_file(const char *src, const char *dst, int level, int single_member)
{
    if (!src || !dst) return PC_ERR_BAD_ARG;
    level = pcz::default_level(level);
    const int fd = open(src, O_RDONLY);
    if (fd < 0) return PC_ERR_BAD_ARG;
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); return PC_ERR_BAD_ARG; }
    const size_t size = (size_t)st.st_size;
    void *m = size ? mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
    close(fd);
    if (size && m == MAP_FAILED) return PC_ERR_BAD_ARG;
    const char *base = (const char *)m;
    const size_t unit = single_member ? ((size_t)1 << 20) : (pcz::kBlockIn * 16);
    const size_t nunits = (size + unit - 1) / unit;
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)usable_threads(), nunits));
    // units are compressed in batches of 4 T, written in order after each batch (memory: a few MB per thread)
    const int ofd = open(dst, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (ofd < 0) { if (m) munmap(m, size); return PC_ERR_BAD_ARG; }
    bool ok = true;
    auto put = [&](const void *p, size_t n) {
        const char *c = (const char *)p;
        while (n && ok) { const ssize_t w = write(ofd, c, n); if (w <= 0) { ok = false; break; } c += w; n -= (size_t)w; }
    };
    uLong crc = crc32(0L, Z_NULL, 0);
    if (single_member) { const unsigned char hdr[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff}; put(hdr, 10); }
    const size_t batch = (size_t)T * 4;
    std::vector<std::vector<char>> outs(batch);
    std::vector<uLong> crcs(batch, 0);
    for (size_t u0 = 0; u0 < nunits && ok; u0 += batch) {
        const size_t u1 = std::min(nunits, u0 + batch);
        std::atomic<size_t> next{u0};
        std::atomic<bool> good{true};
        auto work = [&]() {
            pcz::Deflater def(level);
            z_stream zs;
            memset(&zs, 0, sizeof zs);
            bool z_ok = single_member && deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK;
            for (;;) {
                const size_t u = next.fetch_add(1);
                if (u >= u1) break;
                const char *in = base + u * unit;
                const size_t n = std::min(unit, size - u * unit);
                std::vector<char> &o = outs[u - u0];
                o.clear();
                if (!single_member) {
                    if (!def.usable() || !def.append(in, n, o)) good.store(false);
                    continue;
                }
                if (!z_ok) { good.store(false); continue; }
                deflateReset(&zs);
                o.resize(deflateBound(&zs, (uLong)n) + 64);
                zs.next_in = (Bytef *)in; zs.avail_in = (uInt)n;
                zs.next_out = (Bytef *)o.data(); zs.avail_out = (uInt)o.size();
                const bool last = u + 1 == nunits;
                const int r = deflate(&zs, last ? Z_FINISH : Z_SYNC_FLUSH);
                if ((last && r != Z_STREAM_END) || (!last && (r != Z_OK || zs.avail_in))) good.store(false);
                o.resize(o.size() - zs.avail_out);
                crcs[u - u0] = crc32(crc32(0L, Z_NULL, 0), (const Bytef *)in, (uInt)n);
            }
            if (z_ok) deflateEnd(&zs);
        };
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back(work);
        work();
        for (auto &x : th) x.join();
        if (!good.load()) ok = false;
        for (size_t u = u0; u < u1 && ok; ++u) {
            put(outs[u - u0].data(), outs[u - u0].size());
            if (single_member) crc = crc32_combine(crc, crcs[u - u0], (z_off_t)std::min(unit, size - u * unit));
        }
    }
    if (single_member) {
        if (size == 0) { const unsigned char empty[2] = {3, 0}; put(empty, 2); }
        unsigned char tr[8];
        pcz::put32(tr, (uint32_t)crc); pcz::put32(tr + 4, (uint32_t)(size & 0xffffffffu));
        put(tr, 8);
    } else {
        put(pcz::kEofBlock, sizeof pcz::kEofBlock);
    }
    if (close(ofd) != 0) ok = false;
    if (m) munmap(m, size);
    return ok ? PC_OK : PC_ERR_BAD_ARG;
}

static int write_pieces(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                        const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                        const char *const *file_paths, int fastq, int64_t *bytes_written, int64_t *file_pos, int shared,
                        int64_t *sizes_only, pc_gzimage *image, int gz_level)
{
    if (!rs || npieces < 0 || nfiles < 0 || (npieces > 0 && (!piece_read || !piece_start || !piece_len || !piece_file || !file_paths)))
        return PC_ERR_BAD_ARG;
    const int64_t nreads = (int64_t)rs->off.size();
    for (int64_t k = 0; k < npieces; ++k) {
        const int64_t r = piece_read[k];
        if (r < 0 || r >= nreads || piece_file[k] < 0 || piece_file[k] >= nfiles) return PC_ERR_BAD_ARG;
        if (piece_start[k] < 0 || piece_len[k] < 0 || (int64_t)piece_start[k] + piece_len[k] > rs->len[(size_t)r]) return PC_ERR_BAD_ARG;
    }
    // header: add_number_to_read_name (nanopore_read.py:494-498): "_<k>" before the first space, or at the end
    auto tag_of = [&](int64_t k, char *tag) -> int {
        const int number = piece_number ? piece_number[k] : 0;
        return number > 0 ? snprintf(tag, 24, "_%d", number) : 0;
    };
    auto size_of = [&](int64_t k) -> size_t {
        char tag[24];
        const size_t ln = (size_t)piece_len[k];
        const size_t head = 1 + rs->name_len((size_t)piece_read[k]) + (size_t)tag_of(k, tag) + 1;
        if (fastq) return head + ln + 3 + ln + 1;
        return head + (ln == 0 ? 1 : ln + (ln + 69) / 70);
    };
    auto format = [&](int64_t k, char *o) -> char * {
        const size_t r = (size_t)piece_read[k];
        const size_t st = (size_t)piece_start[k], ln = (size_t)piece_len[k];
        char tag[24];
        const int tl = tag_of(k, tag);
        const char *name = rs->name_of(r);
        const size_t name_n = strlen(name);
        *o++ = fastq ? '@' : '>';
        const char *sp = tl ? (const char *)memchr(name, ' ', name_n) : nullptr;
        if (tl && sp) { memcpy(o, name, (size_t)(sp - name)); o += sp - name; memcpy(o, tag, (size_t)tl); o += tl; memcpy(o, sp, name_n - (size_t)(sp - name)); o += name_n - (size_t)(sp - name); }
        else { memcpy(o, name, name_n); o += name_n; if (tl) { memcpy(o, tag, (size_t)tl); o += tl; } }
        *o++ = '\n';
        const char *seq = rs->arena.data() + rs->off[r] + st;
        const bool rna = rs->rna[r] != 0;
        char *seq_at = o;
        if (fastq) {
            memcpy(o, seq, ln); o += ln;
            *o++ = '\n'; *o++ = '+'; *o++ = '\n';
            if (rs->fastq) memcpy(o, rs->qual_of(r) + st, ln);
            else memset(o, '+', ln);                              // FASTA input: NanoporeRead pads the empty qualities with '+'
            o += ln;
            *o++ = '\n';
            if (rna) for (char *c = seq_at; c < seq_at + ln; ++c) if (*c == 'T') *c = 'U';
        } else {
            // add_line_breaks_to_sequence(seq, 70): every line, the last included, ends in '\n'
            if (ln == 0) *o++ = '\n';
            for (size_t pos = 0; pos < ln; pos += 70) {
                const size_t w = ln - pos < 70 ? ln - pos : 70;
                memcpy(o, seq + pos, w); o += w;
                *o++ = '\n';
            }
            if (rna) for (char *c = seq_at; c < o; ++c) if (*c == 'T') *c = 'U';
        }
        return o;
    };

    int64_t total = 0;
    int rc = PC_OK;
    std::vector<std::vector<int64_t>> of_file((size_t)nfiles);
    for (int64_t k = 0; k < npieces; ++k) of_file[(size_t)piece_file[k]].push_back(k);
    const int nthreads = usable_threads();
    for (int f = 0; f < nfiles && rc == PC_OK; ++f) {
        const std::vector<int64_t> &idx = of_file[(size_t)f];
        if (idx.empty()) continue;                                 // a bin that receives nothing leaves no file
        const char *path = file_paths[f];
        const bool to_stdout = path[0] == '-' && path[1] == '\0';
        // where every piece lands
        std::vector<size_t> at(idx.size() + 1, 0);
        for (size_t i = 0; i < idx.size(); ++i) at[i + 1] = at[i] + size_of(idx[i]);
        const size_t bytes = at.back();
        if (sizes_only) { sizes_only[f] = (int64_t)bytes; continue; }
        if (image) {
            // spans of about equal bytes, one thread each: format a chunk, deflate it, append the members to the span's part
            const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)nthreads, bytes / ((size_t)1 << 20) + 1));
            std::vector<size_t> cut((size_t)T + 1, idx.size());
            cut[0] = 0;
            for (int t = 1; t < T; ++t)
                cut[(size_t)t] = (size_t)(std::lower_bound(at.begin(), at.end(), bytes / (size_t)T * (size_t)t) - at.begin());
            auto &parts = image->parts[(size_t)f];
            parts.assign((size_t)T, std::vector<char>());
            image->plain[(size_t)f] = (int64_t)bytes;
            std::vector<int> ok((size_t)T, 1);
            auto work = [&](int t) {
                pcz::Deflater def(gz_level);
                if (!def.usable()) { ok[(size_t)t] = 0; return; }
                std::vector<char> buf;
                std::vector<char> &z = parts[(size_t)t];
                size_t i = cut[(size_t)t];
                const size_t stop = std::max(cut[(size_t)t], cut[(size_t)t + 1]);
                z.reserve((at[stop] - at[i]) / 2 + 4096);
                // chunks of whole members (16 x 65 280 bytes): only a span's last member is short
                const size_t chunk = pcz::kBlockIn * 16;
                size_t have = 0;                                  // bytes of buf not yet deflated
                buf.resize(chunk + ((size_t)1 << 16));
                while (i < stop) {
                    const size_t need = size_of(idx[i]);
                    if (have + need > buf.size()) buf.resize(std::max(buf.size() * 2, have + need));
                    char *o = format(idx[i], buf.data() + have);
                    if ((size_t)(o - (buf.data() + have)) != need) { ok[(size_t)t] = 0; return; }
                    have += need; ++i;
                    if (have >= chunk) {
                        const size_t whole = have / pcz::kBlockIn * pcz::kBlockIn;
                        if (!def.append(buf.data(), whole, z)) { ok[(size_t)t] = 0; return; }
                        memmove(buf.data(), buf.data() + whole, have - whole);
                        have -= whole;
                    }
                }
                if (have && !def.append(buf.data(), have, z)) ok[(size_t)t] = 0;
            };
            std::vector<std::thread> th;
            for (int t = 1; t < T; ++t) th.emplace_back(work, t);
            work(0);
            for (auto &x : th) x.join();
            for (int t = 0; t < T; ++t) if (!ok[(size_t)t]) rc = PC_ERR_BAD_ARG;
            total += (int64_t)bytes;
            continue;
        }
        if (to_stdout) {
            std::vector<char> buf;
            for (size_t i = 0; i < idx.size() && rc == PC_OK; ) {
                size_t j = i;
                while (j < idx.size() && at[j + 1] - at[i] <= ((size_t)1 << 24)) ++j;
                if (j == i) j = i + 1;
                buf.resize(at[j] - at[i]);
                char *o = buf.data();
                for (size_t q = i; q < j; ++q) o = format(idx[q], o);
                if (fwrite(buf.data(), 1, buf.size(), stdout) != buf.size()) rc = PC_ERR_BAD_ARG;
                i = j;
            }
            fflush(stdout);
        } else {
            const size_t base_pos = file_pos ? (size_t)file_pos[f] : 0;
            // shared: several processes write disjoint spans of one file (a sharded run): never truncate, whatever the position
            const int fd = open(path, shared ? (O_RDWR | O_CREAT) : (base_pos ? O_RDWR : (O_RDWR | O_CREAT | O_TRUNC)), 0666);
            if (fd < 0) { rc = PC_ERR_BAD_ARG; break; }
            // Threads format their spans in parallel; their pwrite()s take turns on a mutex of ours.  Writes to ONE file
            // are serialised by the inode's lock anyway, and on the GPU box 16 threads fighting over that lock move
            // 3.4 GB/s (tmpfs) / 12.5 GB/s (page cache) where a single writer moves 8.9 / 15 GB/s
            // (tools/ubench_write.cpp).  Formatting straight into a shared mapping of the file (PC_IO_MMAP=1) is faster
            // on some kernels (4x in the build container) and slower on that box (page faults on one file: 2-4 GB/s),
            // so it is opt-in; it is only used when the filesystem has the room (a fault on a full filesystem is a
            // SIGBUS, a failed pwrite an error code).
            char *map = nullptr;
            size_t map_len = 0, map_lead = 0;
            static const bool use_mmap = [] { const char *e = getenv("PC_IO_MMAP"); return e && *e && *e != '0'; }();
            std::mutex write_turn;
            // (never for a file other processes write spans of: the ftruncate below would cut a higher rank's span off)
            if (use_mmap && !shared && bytes >= ((size_t)1 << 22)) {
                struct statvfs sv;
                if (fstatvfs(fd, &sv) == 0 && (unsigned long long)sv.f_bavail * (unsigned long long)sv.f_frsize > (unsigned long long)bytes + ((unsigned long long)256 << 20) &&
                    ftruncate(fd, (off_t)(base_pos + bytes)) == 0) {
                    const size_t pg = (size_t)sysconf(_SC_PAGESIZE);
                    const size_t map_off = base_pos & ~(pg - 1);
                    map_lead = base_pos - map_off;
                    void *m = mmap(nullptr, map_lead + bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, (off_t)map_off);
                    if (m != MAP_FAILED) { map = (char *)m; map_len = map_lead + bytes; }
                }
            }
            // spans of pieces with about equal bytes, formatted by one thread each and written in place
            const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)nthreads, bytes / ((size_t)1 << 22) + 1));
            std::vector<size_t> cut((size_t)T + 1, idx.size());
            cut[0] = 0;
            for (int t = 1; t < T; ++t)
                cut[(size_t)t] = (size_t)(std::lower_bound(at.begin(), at.end(), bytes / (size_t)T * (size_t)t) - at.begin());
            std::vector<int> ok((size_t)T, 1);
            // the gather path (PC_IO_GATHER=1): FASTQ out of a FASTQ read set, no RNA read among the pieces (U for T needs a
            // copy), records long enough that five vectors per record are few.
            // Measured on the GPU box (6.4 GB into one file through the page cache): SLOWER than the buffered path, 0.80
            // against 0.58 s -- writes to one file are serialised by the inode's lock, and a gather of five vectors per
            // record lengthens exactly that section, while the buffered path gathers outside it, in parallel.  Opt-in.
            static const bool gather_on = [] { const char *e = getenv("PC_IO_GATHER"); return e && *e && *e != '0'; }();
            bool gather_write = gather_on && fastq && rs->fastq && !map && bytes / idx.size() >= 1024;
            if (gather_write)
                for (int64_t k : idx) if (rs->rna[(size_t)piece_read[k]]) { gather_write = false; break; }
            auto work = [&](int t) {
                std::vector<char> buf;
                size_t i = cut[(size_t)t];
                const size_t stop = std::max(cut[(size_t)t], cut[(size_t)t + 1]);
                if (map) {
                    char *o = map + map_lead + at[i];
                    for (size_t q = i; q < stop; ++q) o = format(idx[q], o);
                    if ((size_t)(o - (map + map_lead)) != at[stop]) ok[(size_t)t] = 0;
                    return;
                }
                if (gather_write) {
                    // FASTQ records of a FASTQ read set: the sequence and quality bytes are written straight from the arenas
                    // (pwritev), only the header lines are formatted -- one copy of every output byte fewer on a path that
                    // is bound by memory copies (the page-cache copy of the write itself remains, serialised per file)
                    static const char sep[] = "\n+\n", nl[] = "\n";
                    std::vector<struct iovec> iov;
                    std::vector<char> hdr;
                    while (i < stop) {
                        size_t j = i;
                        while (j < stop && j - i < 200 && at[j + 1] - at[i] <= ((size_t)1 << 24)) ++j;     // 5 vectors per record, IOV_MAX 1024
                        if (j == i) j = i + 1;
                        size_t hbytes = 0;
                        for (size_t q = i; q < j; ++q) hbytes += size_of(idx[q]) - 2 * (size_t)piece_len[idx[q]] - 4;
                        hdr.resize(hbytes);
                        iov.clear();
                        char *o = hdr.data();
                        for (size_t q = i; q < j; ++q) {
                            const int64_t k = idx[q];
                            const size_t r = (size_t)piece_read[k], st = (size_t)piece_start[k], ln = (size_t)piece_len[k];
                            char tag[24];
                            const int tl = tag_of(k, tag);
                            const char *name = rs->name_of(r);
                            const size_t name_n = strlen(name);
                            char *h0 = o;
                            *o++ = '@';
                            const char *sp = tl ? (const char *)memchr(name, ' ', name_n) : nullptr;
                            if (tl && sp) { memcpy(o, name, (size_t)(sp - name)); o += sp - name; memcpy(o, tag, (size_t)tl); o += tl; memcpy(o, sp, name_n - (size_t)(sp - name)); o += name_n - (size_t)(sp - name); }
                            else { memcpy(o, name, name_n); o += name_n; if (tl) { memcpy(o, tag, (size_t)tl); o += tl; } }
                            *o++ = '\n';
                            iov.push_back({h0, (size_t)(o - h0)});
                            if (ln) iov.push_back({(void *)(rs->arena.data() + rs->off[r] + st), ln});
                            iov.push_back({(void *)sep, 3});
                            if (ln) iov.push_back({(void *)(rs->qual_of(r) + st), ln});
                            iov.push_back({(void *)nl, 1});
                        }
                        if ((size_t)(o - hdr.data()) != hbytes) { ok[(size_t)t] = 0; return; }
                        size_t done = 0, first = 0;
                        const size_t total = at[j] - at[i];
                        std::lock_guard<std::mutex> turn(write_turn);
                        while (done < total) {
                            const ssize_t w = pwritev(fd, iov.data() + first, (int)std::min<size_t>(iov.size() - first, 1024),
                                                      (off_t)(base_pos + at[i] + done));
                            if (w <= 0) { ok[(size_t)t] = 0; return; }
                            done += (size_t)w;
                            size_t left = (size_t)w;                              // a short write: skip what has been written
                            while (first < iov.size() && left >= iov[first].iov_len) left -= iov[first++].iov_len;
                            if (left) { iov[first].iov_base = (char *)iov[first].iov_base + left; iov[first].iov_len -= left; }
                        }
                        i = j;
                    }
                    return;
                }
                // chunk of one formatted buffer / one pwrite: small enough to still sit in the core's caches when the
                // kernel copies it under the file's lock (PC_IO_CHUNK_KB; measured on the GPU box, 6.4 GB into one file:
                // 0.5 MB 0.69 s, 2 MB 0.56 s, 8 MB 0.61 s, 32 MB 0.75 s)
                static const size_t chunk_bytes = [] { const char *e = getenv("PC_IO_CHUNK_KB"); const long v = e ? atol(e) : 0; return (size_t)(v > 0 ? v : 2048) << 10; }();
                while (i < stop) {
                    size_t j = i;
                    while (j < stop && at[j + 1] - at[i] <= chunk_bytes) ++j;
                    if (j == i) j = i + 1;
                    buf.resize(at[j] - at[i]);
                    char *o = buf.data();
                    for (size_t q = i; q < j; ++q) o = format(idx[q], o);
                    if ((size_t)(o - buf.data()) != buf.size()) { ok[(size_t)t] = 0; return; }
                    size_t done = 0;
                    std::lock_guard<std::mutex> turn(write_turn);
                    while (done < buf.size()) {
                        const ssize_t w = pwrite(fd, buf.data() + done, buf.size() - done, (off_t)(base_pos + at[i] + done));
                        if (w <= 0) { ok[(size_t)t] = 0; return; }
                        done += (size_t)w;
                    }
                    i = j;
                }
            };
            std::vector<std::thread> th;
            for (int t = 1; t < T; ++t) th.emplace_back(work, t);
            work(0);
            for (auto &x : th) x.join();
            for (int t = 0; t < T; ++t) if (!ok[(size_t)t]) rc = PC_ERR_BAD_ARG;
            if (map && munmap(map, map_len) != 0) rc = PC_ERR_BAD_ARG;
            if (close(fd) != 0) rc = PC_ERR_BAD_ARG;
            if (file_pos) file_pos[f] = (int64_t)(base_pos + bytes);
        }
        total += (int64_t)bytes;
    }
    if (bytes_written) *bytes_written = total;
    return rc;
}

}  // extern "C"
