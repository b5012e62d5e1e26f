// CPU check of the block-strided copy's host split (sos_amd/csrc/blockcopy_plan.h): for
// every element size, block size, block count, stride pair and pair of base
// misalignments of the sweep below, a CPU interpreter walks the plan exactly as the
// kernel's workgroups do (the same bc_split / bc_body_offset / bc_edge_offset) and must
//   * move exactly the bytes of the definition: block i of the target equals block i of
//     the source, every target byte written once;
//   * touch no byte outside a block: each access lies inside one source block and one
//     target block (the buffers are allocated to the exact extents, so AddressSanitizer
//     sees any overhang past either end);
//   * keep every access aligned to its width (unaligned 16-B loads: to 4 B);
//   * name the regime the geometry calls for.
// Built and run by tests/test_blockcopy_plan.py, plain and with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "blockcopy_plan.h"

using namespace sos;

namespace {

struct Case {
    uint64_t es, bsize, nblocks, dstr, sstr, dmis, smis;
};

struct Tally {
    long cases = 0, failed = 0;
    long regime[6] = {};
    long ul = 0;
    char first[512] = {};
};

void fail(Tally &t, const Case &c, const char *what)
{
    if (!t.failed++)
        snprintf(t.first, sizeof(t.first), "es=%llu bsize=%llu nblocks=%llu dst_stride=%llu src_stride=%llu "
                 "dmis=%llu smis=%llu: %s", (unsigned long long)c.es, (unsigned long long)c.bsize,
                 (unsigned long long)c.nblocks, (unsigned long long)c.dstr, (unsigned long long)c.sstr,
                 (unsigned long long)c.dmis, (unsigned long long)c.smis, what);
}

// One access of `width` bytes at block-relative positions; false if it leaves a block.
struct Mover {
    const Case &c;
    const BcPlan &p;
    unsigned char *dst;
    const unsigned char *src;
    uint64_t moved = 0;
    const char *err = nullptr;
    void move(uint64_t blk, uint64_t in, uint64_t width, uint64_t load_align)
    {
        if (blk >= p.nblocks || in + width > p.bbytes) {
            err = "access outside its block";
            return;
        }
        const unsigned char *s = src + blk * p.sstride_b + in;
        unsigned char *d = dst + blk * p.dstride_b + in;
        if ((uintptr_t)s % load_align || (uintptr_t)d % width) {
            err = "misaligned access";
            return;
        }
        for (uint64_t k = 0; k < width; ++k)
            if (d[k]) err = "target byte written twice";
        memcpy(d, s, width);
        moved += width;
    }
};

void run_case(const Case &c, Tally &t)
{
    ++t.cases;
    const uint64_t bbytes = c.bsize * c.es;
    const uint64_t sext = ((c.nblocks - 1) * c.sstr + c.bsize) * c.es;
    const uint64_t dext = ((c.nblocks - 1) * c.dstr + c.bsize) * c.es;
    // exact extents behind a base of the wanted misalignment; zero = never written
    unsigned char *sbuf = (unsigned char *)malloc(c.smis + sext);
    unsigned char *dbuf = (unsigned char *)calloc(1, c.dmis + dext);
    if (!sbuf || !dbuf || (uintptr_t)sbuf % 16 || (uintptr_t)dbuf % 16) {
        fail(t, c, "no 16-B aligned memory");
        free(sbuf);
        free(dbuf);
        return;
    }
    unsigned char *src = sbuf + c.smis, *dst = dbuf + c.dmis;
    for (uint64_t i = 0; i < c.nblocks; ++i)
        for (uint64_t k = 0; k < bbytes; ++k)
            src[i * c.sstr * c.es + k] = (unsigned char)(1 + (i * 131 + k * 7 + c.smis) % 255);  // never 0
    BcPlan p;
    const int rc = bc_plan(&p, (uintptr_t)dst, (ptrdiff_t)c.dstr, (uintptr_t)src, (ptrdiff_t)c.sstr, c.bsize,
                           c.nblocks, c.es);
    if (rc != 0) {
        fail(t, c, "bc_plan refused the call");
    } else {
        // the regime the geometry calls for
        const uint64_t sb = c.sstr * c.es, db = c.dstr * c.es;
        int want;
        if (c.nblocks == 1 || (c.sstr == c.bsize && c.dstr == c.bsize)) want = BC_CONTIGUOUS;
        else if (bbytes < 16) want = -1;  // small or delegated: checked below
        else if (sb % 16 == 0 && db % 16 == 0 && ((uintptr_t)src - (uintptr_t)dst) % 16 == 0) want = BC_CONGRUENT;
        else want = BC_INCONGRUENT;
        if (want >= 0 && p.regime != want) fail(t, c, "wrong regime");
        if (want < 0 && p.regime != BC_SMALL && p.regime != BC_ELEMENT) fail(t, c, "wrong regime (small block)");
        if (p.regime >= 0 && p.regime < 6) ++t.regime[p.regime];
        Mover m{c, p, dst, src};
        if (p.regime == BC_CONTIGUOUS || p.regime == BC_ELEMENT) {
            // sosx_strided_copy(dst, d_dstr, src, d_sstr, d_es, d_count)
            if ((uintptr_t)dst % p.d_es || (uintptr_t)src % p.d_es || p.d_dstr < 1 || p.d_sstr < 1)
                fail(t, c, "delegated call breaks sosx_strided_copy's contract");
            if (p.regime == BC_ELEMENT && p.d_dstr != 1 && p.d_sstr != 1) fail(t, c, "no contiguous side");
            for (uint64_t k = 0; k < p.d_count && !m.err; ++k) {
                const unsigned char *s = src + k * (uint64_t)p.d_sstr * p.d_es;
                unsigned char *d = dst + k * (uint64_t)p.d_dstr * p.d_es;
                if (s < src || s + p.d_es > src + sext || d < dst || d + p.d_es > dst + dext) {
                    m.err = "delegated access outside the extents";
                    break;
                }
                memcpy(d, s, p.d_es);
                m.moved += p.d_es;
            }
        } else {
            if (p.regime == BC_CONGRUENT && (p.width != 16 || p.unaligned_loads)) fail(t, c, "congruent: not 16-B");
            if (p.regime == BC_SMALL && p.width != p.es) fail(t, c, "small: width != element");
            if (p.head >= 16 || p.tail >= 16 || p.head + p.upb * p.width + p.tail != p.bbytes)
                fail(t, c, "head + body + tail != block");
            if (p.unaligned_loads) ++t.ul;
            const uint64_t la = p.unaligned_loads ? 4 : p.width;
            const uint64_t wgs = p.body_wgs + p.edge_wgs;
            for (uint64_t wg = 0; wg < wgs && !m.err; ++wg) {
                if (wg < p.body_wgs) {
                    const uint64_t w0 = wg * kBcTile;
                    for (uint32_t off = 0; off < kBcTile && w0 + off < p.body_units; ++off) {
                        const BcItem it = bc_split(w0, off, p.upb);
                        if (it.blk * p.upb + it.j != w0 + off) m.err = "bc_split is not the flat numbering";
                        m.move(it.blk, bc_body_offset(p, it.j), p.width, la);
                    }
                } else {
                    const uint64_t e0 = (wg - p.body_wgs) * kBcTile;
                    for (uint32_t off = 0; off < kBcTile && e0 + off < p.edge_units; ++off) {
                        const BcItem it = bc_split(e0, off, p.epb);
                        m.move(it.blk, bc_edge_offset(p, it.j), p.es, p.es);
                    }
                }
            }
        }
        if (m.err) fail(t, c, m.err);
        if (m.moved != c.nblocks * bbytes) fail(t, c, "bytes moved != nblocks * block bytes");
        for (uint64_t i = 0; i < c.nblocks; ++i)
            if (memcmp(dst + i * db, src + i * sb, bbytes)) {
                fail(t, c, "a target block differs from its source block");
                break;
            }
        // the gap bytes next to the target blocks kept their zeros (the blocks hold none;
        // every access was already checked to lie inside a block)
        if (c.dstr > c.bsize)
            for (uint64_t i = 0; i + 1 < c.nblocks; ++i) {
                const unsigned char *g = dst + i * db + bbytes;
                const uint64_t n = db - bbytes, near = n < 32 ? n : 32;
                for (uint64_t k = 0; k < near; ++k)
                    if (g[k] || g[n - 1 - k]) fail(t, c, "a gap byte was written");
            }
        for (uint64_t k = 0; k < c.dmis; ++k)
            if (dbuf[k]) fail(t, c, "a byte before the target was written");
    }
    free(sbuf);
    free(dbuf);
}

struct Task {
    uint64_t es, bsize, nblocks;
};

std::vector<Task> tasks()
{
    std::vector<Task> out;
    for (uint64_t es : {1, 2, 4, 8, 16}) {
        const uint64_t V = 16 / es;
        std::vector<uint64_t> bsizes;
        for (uint64_t b : {(uint64_t)1, (uint64_t)2, (uint64_t)3, V - 1, V, V + 1, 64 * V - 1, 64 * V, 64 * V + 5}) {
            bool seen = b == 0;
            for (uint64_t x : bsizes) seen |= x == b;
            if (!seen) bsizes.push_back(b);
        }
        for (uint64_t bsize : bsizes)
            for (uint64_t nblocks : {257, 3, 2, 1}) out.push_back(Task{es, bsize, nblocks});
    }
    return out;
}

void sweep(const Task &k, Tally &t)
{
    const uint64_t V = 16 / k.es;
    // bsize, bsize + 1, a multiple of 16 B past the block, 4099
    const uint64_t strides[4] = {k.bsize, k.bsize + 1, (k.bsize / V + 2) * V, 4099};
    for (uint64_t dstr : strides)
        for (uint64_t sstr : strides)
            for (uint64_t dmis = 0; dmis < 16; dmis += k.es)
                for (uint64_t smis = 0; smis < 16; smis += k.es)
                    run_case(Case{k.es, k.bsize, k.nblocks, dstr, sstr, dmis, smis}, t);
}

int refusals()
{
    BcPlan p;
    int bad = 0;
    bad += bc_plan(&p, 64, 4, 128, 4, 4, 2, 3) != -3;     // element size
    bad += bc_plan(&p, 64, 3, 128, 4, 4, 2, 4) != -3;     // target stride < bsize
    bad += bc_plan(&p, 64, 4, 128, 3, 4, 2, 4) != -3;     // source stride < bsize
    bad += bc_plan(&p, 64, -4, 128, 4, 4, 2, 4) != -3;    // negative stride
    bad += bc_plan(&p, 0, 4, 128, 4, 4, 2, 4) != -3;      // null target
    bad += bc_plan(&p, 64, 4, 0, 4, 4, 2, 4) != -3;       // null source
    bad += bc_plan(&p, 66, 4, 128, 4, 4, 2, 4) != -3;     // target not element-aligned
    bad += bc_plan(&p, 64, (ptrdiff_t)1 << 40, 128, 4, 4, (size_t)1 << 40, 4) != -3;  // extent overflows
    bad += !(bc_plan(&p, 0, 4, 0, 4, 0, 2, 4) == 0 && p.regime == BC_EMPTY);  // bsize 0: a no-op
    bad += !(bc_plan(&p, 0, 4, 0, 4, 4, 0, 4) == 0 && p.regime == BC_EMPTY);  // nblocks 0: a no-op
    return bad;
}

}  // namespace

int main()
{
    const std::vector<Task> todo = tasks();
    std::vector<Tally> t(todo.size());
    std::atomic<size_t> next{0};
    unsigned nth = std::thread::hardware_concurrency();
    nth = nth < 1 ? 1 : nth > 16 ? 16 : nth;
    std::vector<std::thread> th;
    for (unsigned i = 0; i < nth; ++i)
        th.emplace_back([&] {
            for (size_t k; (k = next++) < todo.size();) sweep(todo[k], t[k]);
        });
    for (auto &x : th) x.join();
    long cases = 0, failed = 0, ul = 0, regime[6] = {};
    for (size_t i = 0; i < t.size(); ++i) {
        cases += t[i].cases;
        failed += t[i].failed;
        ul += t[i].ul;
        for (int r = 0; r < 6; ++r) regime[r] += t[i].regime[r];
        if (t[i].failed) printf("FAILED (%ld cases), first: %s\n", t[i].failed, t[i].first);
    }
    const int bad = refusals();
    if (bad) printf("FAILED: %d argument checks\n", bad);
    for (int r = BC_CONTIGUOUS; r <= BC_INCONGRUENT; ++r)
        if (!regime[r]) {
            printf("FAILED: regime %d never chosen\n", r);
            ++failed;
        }
    if (!ul) {
        printf("FAILED: the unaligned-load form never chosen\n");
        ++failed;
    }
    if (failed || bad) return 1;
    printf("block copy plans OK: %ld cases (contiguous %ld, element %ld, small %ld, congruent %ld, "
           "incongruent %ld of which %ld with unaligned loads)\n", cases, regime[1], regime[2], regime[3],
           regime[4], regime[5], ul);
    return 0;
}
