// CPU check of the gather's host split (sos_amd/csrc/gather_plan.h): for every case of the
// sweep below a CPU interpreter walks every launch exactly as k_gather's workgroups do
// (copy.hip: one tile of kTileVec vectors per workgroup in one of three load forms, plus
// the last workgroup's byte loops for the heads and tails) and must find that
//   * every destination byte of every live segment is written exactly once over the whole
//     call and equals its source byte, and no byte outside a destination is written;
//   * every store and every unaligned load lies wholly inside its segment;
//   * every aligned 16-B load is 16-B aligned and holds at least one byte of its segment
//     (the load is modelled as reading only those bytes: the buffers have the exact
//     extents, so AddressSanitizer sees anything else);
//   * no unaligned load is off a 4-B boundary;
//   * tstart is the prefix sum of the tiles and the grid is max(1, tiles);
//   * the segment slots over all launches equal the live segments, each segment in one
//     launch;
//   * the gate is fused only when all live segments fit one launch of at most
//     kGateMaxBlocks workgroups, otherwise its own step before the first copy, and its
//     own step alone when nothing is copied.
// Built and run by tests/test_gather_plan.py, plain and with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "gather_plan.h"

using namespace sos;

namespace {

struct Seg {
    uint64_t so, doff, bytes;  // source / destination offset mod 16, length
};

struct Case {
    std::string name;
    std::vector<Seg> segs;
    bool ul, gated;
};

struct Tally {
    long cases = 0, failed = 0;
    long gate[4] = {};
    long tiles_step = 0;  // one launch whose tiles alone put the gate into its own step
    long multi = 0;       // calls of more than one launch
    long form[3] = {};    // tiles walked: congruent, unaligned loads, DPP
    char first[768] = {};
};

struct Buf {  // one segment's memory: exact extents behind 16-B aligned bases
    unsigned char *sbase = nullptr, *dbase = nullptr, *wrote = nullptr;
    const unsigned char *src = nullptr;
    unsigned char *dst = nullptr;
    uint64_t bytes = 0;
    int placed = 0;
};

struct Vec {  // a 16-B register: its bytes and which of them a load really fetched
    unsigned char b[16];
    bool ok[16];
};

struct Walker {
    const Case &c;
    Tally &t;
    std::vector<Buf> buf;
    bool bad = false;

    Walker(const Case &c_, Tally &t_) : c(c_), t(t_) {}

    void fail(const char *what, int seg = -1, long long at = -1, int launch = -1)
    {
        bad = true;
        if (t.failed++) return;
        char where[160] = "";
        if (seg >= 0)
            snprintf(where, sizeof(where), " [segment %d of %zu (src+%llu, dst+%llu, %llu bytes), byte %lld, launch %d]",
                     seg, c.segs.size(), (unsigned long long)c.segs[seg].so, (unsigned long long)c.segs[seg].doff,
                     (unsigned long long)c.segs[seg].bytes, at, launch);
        snprintf(t.first, sizeof(t.first), "%s ul=%d gated=%d: %s%s", c.name.c_str(), (int)c.ul, (int)c.gated, what,
                 where);
    }

    // An aligned 16-B load at segment-relative source offset `off` (it may begin before the
    // segment or end after it): only the segment's own bytes are read.
    Vec load_aligned(int s, int64_t off, int launch)
    {
        Vec v = {};
        const Buf &m = buf[s];
        if (((uintptr_t)m.src + (uintptr_t)off) % 16) fail("aligned load off the 16-B grid", s, off, launch);
        int held = 0;
        for (int k = 0; k < 16; ++k) {
            const int64_t at = off + k;
            if (at < 0 || at >= (int64_t)m.bytes) continue;
            v.b[k] = m.src[at];
            v.ok[k] = true;
            ++held;
        }
        if (!held) fail("aligned load holds no byte of its segment", s, off, launch);
        return v;
    }

    Vec load_unaligned(int s, int64_t off, int launch)
    {
        Vec v = {};
        const Buf &m = buf[s];
        if (off < 0 || off + 16 > (int64_t)m.bytes) {
            fail("unaligned load leaves its segment", s, off, launch);
            return v;
        }
        if (((uintptr_t)m.src + (uintptr_t)off) % 4) fail("unaligned load off the 4-B grid", s, off, launch);
        for (int k = 0; k < 16; ++k) {
            v.b[k] = m.src[off + k];
            v.ok[k] = true;
        }
        return v;
    }

    void store_byte(int s, uint64_t at, unsigned char val, int launch)
    {
        Buf &m = buf[s];
        if (at >= m.bytes) {
            fail("store outside its segment", s, (long long)at, launch);
            return;
        }
        if (m.wrote[at]++) fail("destination byte written twice", s, (long long)at, launch);
        m.dst[at] = val;
    }

    void store_vec(int s, uint64_t off, const Vec &v, int launch)
    {
        Buf &m = buf[s];
        if (off + 16 > m.bytes) {
            fail("16-B store leaves its segment", s, (long long)off, launch);
            return;
        }
        if (((uintptr_t)m.dst + off) % 16) fail("16-B store off the 16-B grid", s, (long long)off, launch);
        for (int k = 0; k < 16; ++k) {
            if (!v.ok[k]) fail("a stored byte was never loaded", s, (long long)off + k, launch);
            store_byte(s, off + k, v.b[k], launch);
        }
    }

    // k_gather, workgroup `wg` of `grid`
    void workgroup(const GatherLaunch &g, uint64_t wg, uint64_t grid, int launch)
    {
        const uint64_t t0 = wg;  // blockIdx.x
        if (t0 < g.tstart[g.nseg]) {
            int n = 0;
            while (t0 >= g.tstart[n + 1]) ++n;
            const int s = g.seg[n];
            const unsigned sd = g.sd[n];
            const int64_t sbody = (int64_t)g.head[n] - (int64_t)sd;  // src + head - sd
            const uint64_t nv = g.nvec[n];
            const uint64_t jbase = (t0 - g.tstart[n]) * kTileVec;
            static Vec v[kGatherThreads][kGatherU], lo[kGatherThreads][kGatherU], hi[kGatherThreads][kGatherU];
            const Vec none = {};
            for (unsigned tid = 0; tid < kGatherThreads; ++tid)
                for (int u = 0; u < kGatherU; ++u) v[tid][u] = lo[tid][u] = hi[tid][u] = none;
            if (sd == 0) {
                ++t.form[0];
                for (unsigned tid = 0; tid < kGatherThreads; ++tid)
                    for (int u = 0; u < kGatherU; ++u) {
                        const uint64_t j = jbase + tid + (uint64_t)u * kGatherThreads;
                        if (j < nv) v[tid][u] = load_aligned(s, sbody + (int64_t)j * 16, launch);
                    }
            } else if (g.ul && (sd & 3) == 0) {
                ++t.form[1];
                for (unsigned tid = 0; tid < kGatherThreads; ++tid)
                    for (int u = 0; u < kGatherU; ++u) {
                        const uint64_t j = jbase + tid + (uint64_t)u * kGatherThreads;
                        if (j < nv) v[tid][u] = load_unaligned(s, sbody + (int64_t)j * 16 + sd, launch);
                    }
            } else {
                ++t.form[2];
                for (unsigned tid = 0; tid < kGatherThreads; ++tid)
                    for (int u = 0; u < kGatherU; ++u) {
                        const uint64_t j = jbase + tid + (uint64_t)u * kGatherThreads;
                        if (j <= nv) lo[tid][u] = load_aligned(s, sbody + (int64_t)j * 16, launch);
                    }
                for (unsigned tid = 0; tid < kGatherThreads; ++tid) {
                    const bool last_lane = (tid & 63) == 63;
                    for (int u = 0; u < kGatherU; ++u) {
                        const uint64_t j = jbase + tid + (uint64_t)u * kGatherThreads;
                        if (last_lane) {
                            if (j < nv) hi[tid][u] = load_aligned(s, sbody + (int64_t)(j + 1) * 16, launch);
                        } else {
                            hi[tid][u] = lo[tid + 1][u];  // next_lane16: the next lane's vector j
                        }
                        if (j < nv)  // realign16: bytes sd .. sd + 15 of lo || hi
                            for (int k = 0; k < 16; ++k) {
                                const Vec &from = sd + k < 16 ? lo[tid][u] : hi[tid][u];
                                v[tid][u].b[k] = from.b[(sd + k) & 15];
                                v[tid][u].ok[k] = from.ok[(sd + k) & 15];
                            }
                    }
                }
            }
            for (unsigned tid = 0; tid < kGatherThreads; ++tid)
                for (int u = 0; u < kGatherU; ++u) {
                    const uint64_t j = jbase + tid + (uint64_t)u * kGatherThreads;
                    if (j < nv) store_vec(s, g.head[n] + j * 16, v[tid][u], launch);
                }
        }
        if (wg == grid - 1)  // ragged ends: the last workgroup copies them byte by byte
            for (int n = 0; n < g.nseg; ++n) {
                const int s = g.seg[n];
                for (uint64_t b = 0; b < g.head[n]; ++b) store_byte(s, b, byte_of(s, b, launch), launch);
                for (uint64_t b = g.head[n] + g.nvec[n] * 16; b < g.bytes[n]; ++b)
                    store_byte(s, b, byte_of(s, b, launch), launch);
            }
    }

    unsigned char byte_of(int s, uint64_t at, int launch)
    {
        if (at >= buf[s].bytes) {
            fail("byte load outside its segment", s, (long long)at, launch);
            return 0;
        }
        return buf[s].src[at];
    }

    void geometry(const GatherLaunch &g, int launch)
    {
        if (g.nseg < 1 || g.nseg > kMaxSeg) {
            fail("a launch of no or too many segments");
            return;
        }
        uint64_t tot = 0;
        for (int n = 0; n < g.nseg; ++n) {
            const int s = g.seg[n];
            if (s < 0 || s >= (int)buf.size() || !buf[s].bytes) {
                fail("a slot names no live segment");
                return;
            }
            const Buf &m = buf[s];
            if (g.bytes[n] != m.bytes) fail("bytes differ from the segment's", s, 0, launch);
            if (g.head[n] > 15 || g.head[n] + g.nvec[n] * 16 > m.bytes || m.bytes - g.head[n] - g.nvec[n] * 16 > 15)
                fail("head + body + tail != segment", s, 0, launch);
            if (g.nvec[n] && ((uintptr_t)m.dst + g.head[n]) % 16) fail("body off dst's 16-B grid", s, 0, launch);
            if (g.sd[n] != ((uintptr_t)m.src + g.head[n]) % 16) fail("sd is not src's offset at the body", s, 0, launch);
            if (g.tstart[n] != tot) fail("tstart is not the prefix sum of the tiles", s, 0, launch);
            tot += (g.nvec[n] + kTileVec - 1) / kTileVec;
        }
        if (g.tstart[g.nseg] != tot) fail("tstart[nseg] is not the total of the tiles");
        if (g.blocks != (tot ? tot : 1)) fail("grid != max(1, tiles)");
        if (g.ul != (int)c.ul) fail("ul not carried into the launch");
    }

    void run()
    {
        ++t.cases;
        const int nseg = (int)c.segs.size();
        buf.resize(nseg);
        std::vector<const void *> srcs(nseg);
        std::vector<void *> dsts(nseg);
        std::vector<size_t> sizes(nseg);
        int live = 0;
        uint64_t tiles = 0;
        for (int i = 0; i < nseg; ++i) {
            const Seg &g = c.segs[i];
            Buf &m = buf[i];
            m.bytes = g.bytes;
            m.sbase = (unsigned char *)malloc(g.so + g.bytes + !(g.so + g.bytes));
            m.dbase = (unsigned char *)calloc(1, g.doff + g.bytes + !(g.doff + g.bytes));
            m.wrote = (unsigned char *)calloc(1, g.bytes + !g.bytes);
            if (!m.sbase || !m.dbase || !m.wrote || (uintptr_t)m.sbase % 16 || (uintptr_t)m.dbase % 16) {
                fail("no 16-B aligned memory");
                return;
            }
            m.src = m.sbase + g.so;
            m.dst = m.dbase + g.doff;
            for (uint64_t k = 0; k < g.bytes; ++k)
                m.sbase[g.so + k] = (unsigned char)(1 + (i * 131 + k * 7 + g.so) % 255);  // never 0
            srcs[i] = m.src;
            dsts[i] = m.dst;
            sizes[i] = g.bytes;
            if (g.bytes) {
                ++live;
                uint64_t h = (16 - g.doff % 16) % 16;
                if (h > g.bytes) h = g.bytes;
                tiles += ((g.bytes - h) / 16 + kTileVec - 1) / kTileVec;
            }
        }
        // the placement the rule names (tiles: of all live segments, which is one launch's
        // when they fit one)
        int want_gate = GG_NONE;
        if (c.gated)
            want_gate = !live ? GG_STEP_ALONE
                              : live <= kMaxSeg && (tiles ? tiles : 1) <= kGateMaxBlocks ? GG_FUSED : GG_STEP_BEFORE;
        GatherCursor cur = gather_begin(nseg, sizes.data(), c.gated);
        GatherLaunch g;
        int rc, launches = 0, slots = 0, gate = GG_NONE, prev = -1;
        while ((rc = gather_next(&cur, &g, nseg, srcs.data(), dsts.data(), sizes.data(), c.ul)) == 1) {
            geometry(g, launches);
            if (bad) break;
            if (launches ? g.gate != GG_NONE : c.gated == (g.gate == GG_NONE))
                fail("the gate is not placed at the first launch, once");
            if (!launches) gate = g.gate;
            for (uint64_t wg = 0; wg < g.blocks; ++wg) workgroup(g, wg, g.blocks, launches);
            for (int n = 0; n < g.nseg; ++n) {  // after the walk: a repeated segment shows as its bytes first
                if (g.seg[n] <= prev) fail("segments out of order or repeated", g.seg[n], 0, launches);
                prev = g.seg[n];
                if (buf[g.seg[n]].placed++) fail("a segment sits in two launches", g.seg[n], 0, launches);
            }
            slots += g.nseg;
            ++launches;
            if (launches > nseg) {
                fail("more launches than segments");
                break;
            }
        }
        if (rc < 0) fail("gather_next refused the call");
        if (cur.gate_pending) gate = launches ? -1 : GG_STEP_ALONE;
        if (cur.live != live) fail("live count");
        if (slots != live) fail("segment slots over all launches != live segments");
        if (launches != (live + kMaxSeg - 1) / kMaxSeg) fail("launches != ceil(live / kMaxSeg)");
        if (gate != want_gate) fail("wrong gate placement");
        GatherSummary sum;
        if (gather_summary(&sum, nseg, srcs.data(), dsts.data(), sizes.data(), c.gated, c.ul) != 0 ||
            sum.launches != launches || sum.slots != slots || sum.live != live || sum.gate != gate ||
            sum.tiles != (long long)tiles)
            fail("gather_summary disagrees with the launches");
        for (int i = 0; i < nseg; ++i) {
            const Buf &m = buf[i];
            if (m.placed != (m.bytes != 0)) fail("a live segment in no launch, or an empty one in some", i, 0);
            for (uint64_t k = 0; k < m.bytes; ++k)
                if (m.wrote[k] != 1) {
                    fail(m.wrote[k] ? "destination byte written twice" : "destination byte never written", i,
                         (long long)k);
                    break;
                }
            if (m.bytes && memcmp(m.dst, m.src, m.bytes)) fail("a destination differs from its source", i, 0);
            for (uint64_t k = 0; k < c.segs[i].doff; ++k)
                if (m.dbase[k]) fail("a byte before the destination was written", i, -(long long)(c.segs[i].doff - k));
        }
        if (!bad) {
            ++t.gate[gate];
            t.tiles_step += gate == GG_STEP_BEFORE && launches == 1;
            t.multi += launches > 1;
        }
    }

    ~Walker()
    {
        for (Buf &m : buf) {
            free(m.sbase);
            free(m.dbase);
            free(m.wrote);
        }
    }
};

const uint64_t kTileBytes = kTileVec * 16;
const uint64_t kSizes[13] = {0, 1, 15, 16, 17, 31, 32, 33, kTileBytes - 1, kTileBytes, kTileBytes + 1,
                             kTileBytes + 17, 3 * kTileBytes + 5};

void single_segments(Tally &t)
{
    for (uint64_t so = 0; so < 16; ++so)
        for (uint64_t doff = 0; doff < 16; ++doff)
            for (int ul = 0; ul < 2; ++ul)
                for (uint64_t bytes : kSizes) {
                    Case c{"single segment", {Seg{so, doff, bytes}}, ul != 0, false};
                    Walker(c, t).run();
                }
}

void segment_lists(Tally &t)
{
    static const char *const pattern[5] = {"no empties", "first 4 empty", "every other empty", "last 4 empty",
                                           "all empty"};
    for (int nseg : {0, 1, 15, 16, 17, 20, 33, 40})
        for (int p = 0; p < 5; ++p)
            for (int ul = 0; ul < 2; ++ul)
                for (int gated = 0; gated < 2; ++gated) {
                    Case c{std::to_string(nseg) + " segments, " + pattern[p], {}, ul != 0, gated != 0};
                    for (int i = 0; i < nseg; ++i) {
                        const bool empty = p == 1 ? i < 4 : p == 2 ? i % 2 == 0 : p == 3 ? i >= nseg - 4 : p == 4;
                        // sizes and offsets of the single-segment sets, mixed (kSizes[0] is 0)
                        const uint64_t bytes = empty ? 0 : kSizes[1 + (i + nseg) % 12];
                        c.segs.push_back(Seg{(uint64_t)(i * 7 + nseg) % 16, (uint64_t)(i * 11 + 3) % 16, bytes});
                    }
                    Walker(c, t).run();
                }
}

}  // namespace

int main()
{
    Tally t;
    single_segments(t);
    segment_lists(t);
    if (t.failed) printf("FAILED (%ld checks), first: %s\n", t.failed, t.first);
    long failed = t.failed;
    for (int g = GG_NONE; g <= GG_STEP_ALONE; ++g)
        if (!t.gate[g]) {
            printf("FAILED: gate placement %d never seen\n", g);
            ++failed;
        }
    if (!t.tiles_step || !t.multi || !t.form[0] || !t.form[1] || !t.form[2]) {
        printf("FAILED: the sweep misses a path (one launch gated out by its tiles %ld, several launches %ld, "
               "tiles congruent %ld, unaligned %ld, DPP %ld)\n", t.tiles_step, t.multi, t.form[0], t.form[1],
               t.form[2]);
        ++failed;
    }
    if (failed) return 1;
    printf("gather plans OK: %ld cases (ungated %ld, fused %ld, own step before the copies %ld of which %ld in one "
           "launch, own step alone %ld; %ld calls of several launches; tiles walked: congruent %ld, unaligned "
           "loads %ld, DPP %ld)\n", t.cases, t.gate[0], t.gate[1], t.gate[2], t.tiles_step, t.gate[3], t.multi,
           t.form[0], t.form[1], t.form[2]);
    return 0;
}
