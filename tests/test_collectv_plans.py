"""CPU: the collect plans of every PE, decoded through sosx_plan_encode_collect and run by
a byte-buffer simulator in the style of tests/test_collect_plans.py (transfers matched
FIFO per (sender, receiver) pair), against the closed form of SOS's collect
(src/collectives.c:1215-1276):

  target of every PE = concat over q of source(q), source(q) of len[q] bytes
"""
import ctypes

import numpy as np
import pytest

from sos_amd import _lib
from sos_amd import shmem as S

SRC, DST = 0, 1
COPY = 1
ODD = (1, 3, 15, 17, 255)


def _raw(alg, P, me, count, ts, smis=0, dmis=0):
    L = S.lib()
    n = L.sosx_plan_encode(alg, P, me, count, ts, smis, dmis, None, 0)
    assert n > 0
    buf = (ctypes.c_longlong * n)()
    L.sosx_plan_encode(alg, P, me, count, ts, smis, dmis, buf, n)
    return list(buf)


EXISTING = [(2, 5, 1, 4099, 4, 0, 0), (5, 8, 7, 65537, 8, 4, 12), (16, 3, 2, 1001, 4, 0, 8),
            (17, 8, 0, 77, 8, 0, 0), (18, 5, 3, 37, 16, 0, 0), (19, 64, 63, 3, 1, 0, 0),
            (33, 4, 1, 100000, 4, 0, 0), (3, 12, 5, 9999, 2, 0, 0)]
# encoded before this module builds any collect plan
BEFORE = {k: _raw(*k) for k in EXISTING}


def length_vectors(P):
    """name -> per-PE byte lengths."""
    v = {"equal": [37] * P, "zero": [0] * P,
         "one": [0] * (P - 1) + [255] if P > 1 else [255],
         "one_first": [17] + [0] * (P - 1),
         "alternating": [0 if q % 2 == 0 else ODD[(q // 2) % len(ODD)] for q in range(P)],
         "alternating_odd_first": [ODD[(q // 2) % len(ODD)] if q % 2 == 0 else 0 for q in range(P)],
         "long_among_short": [1 + q % 3 for q in range(P)]}
    v["long_among_short"][P // 2] = (1 << 20) + 3
    return v


def simulate(P, lens):
    total = sum(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    plans = [S.plan_collect(P, p, lens) for p in range(P)]
    srcs = [np.random.default_rng(1000 * P + q).integers(0, 256, lens[q], dtype=np.uint8) for q in range(P)]
    TAIL = 32  # bytes above the sum: never written
    bufs = [{SRC: srcs[p], DST: np.full(total + TAIL, 0xA5, dtype=np.uint8)} for p in range(P)]
    writes = [np.zeros(total + TAIL, dtype=np.int32) for _ in range(P)]
    pair_sends, pair_recvs = {}, {}
    for p, pl in enumerate(plans):
        assert pl["alg"] == _lib.PLAN_COLLECT == 20 and pl["scratch_bytes"] == 0
        assert (pl["src_bytes"], pl["dst_bytes"]) == (lens[p], total)
        extent = {SRC: lens[p], DST: total}
        assert len(pl["rounds"]) <= 2
        for r in pl["rounds"]:
            assert r["xfers"] or r["ops"], "empty round"
            for x in r["xfers"]:
                assert x["bytes"] > 0, "empty transfer"
                assert x["buf"] == DST and 0 <= x["peer"] < P and x["peer"] != p
                assert 0 <= x["off"] and x["off"] + x["bytes"] <= extent[x["buf"]], (p, x)
                owner = p if x["send"] else x["peer"]
                assert (x["off"], x["bytes"]) == (off[owner], lens[owner])
                key = (p, x["peer"]) if x["send"] else (x["peer"], p)
                d = pair_sends if x["send"] else pair_recvs
                d.setdefault(key, []).append(x["bytes"])
            for l in r["ops"]:
                assert l["kind"] == COPY and len(l["ins"]) == 1 and l["count"] > 0
                assert (l["ins"][0], l["out"], l["count"]) == ((SRC, 0), (DST, off[p]), lens[p])
        if lens[p] == 0:
            assert not any(r["ops"] for r in pl["rounds"])
            assert not any(x["send"] for r in pl["rounds"] for x in r["xfers"])
    assert pair_sends == pair_recvs, "sends and receives differ for some pair"
    if total == 0:
        assert all(pl["rounds"] == [] for pl in plans)
    fifo = {}
    k = [0] * P
    posted = [False] * P
    outstanding = [0] * P
    done = [None] * P
    while True:
        progress, all_done = False, True
        for p in range(P):
            if k[p] >= len(plans[p]["rounds"]):
                continue
            all_done = False
            r = plans[p]["rounds"][k[p]]
            if not posted[p]:
                for x in r["xfers"]:
                    if x["send"]:
                        data = bufs[p][x["buf"]][x["off"]:x["off"] + x["bytes"]].copy()
                        fifo.setdefault((p, x["peer"]), []).append(data)
                        outstanding[p] += 1
                done[p] = [False] * len(r["xfers"])
                posted[p] = True
                progress = True
            ok = True
            for i, x in enumerate(r["xfers"]):
                if x["send"] or done[p][i]:
                    continue
                q = fifo.get((x["peer"], p), [])
                if not q:
                    ok = False
                    continue
                data = q.pop(0)
                assert data.size == x["bytes"], "plan size mismatch between PEs"
                bufs[p][DST][x["off"]:x["off"] + x["bytes"]] = data
                writes[p][x["off"]:x["off"] + x["bytes"]] += 1
                outstanding[x["peer"]] -= 1
                done[p][i] = True
                progress = True
            if ok and outstanding[p] == 0:
                for l in r["ops"]:
                    (ib, ioff), (ob, ooff), n = l["ins"][0], l["out"], l["count"]
                    bufs[p][ob][ooff:ooff + n] = bufs[p][ib][ioff:ioff + n].copy()
                    writes[p][ooff:ooff + n] += 1
                k[p] += 1
                posted[p] = False
                progress = True
        if all_done:
            break
        assert progress, "plans deadlock"
    assert not any(fifo.values()), "unmatched sends"
    exp = np.concatenate(srcs) if total else np.zeros(0, np.uint8)
    for p in range(P):
        assert np.all(writes[p][:total] == 1), f"PE {p}: a target byte not written exactly once"
        assert not writes[p][total:].any(), f"PE {p}: a byte above the sum written"
        assert np.array_equal(bufs[p][DST][:total], exp), f"collect P={P} lens={lens[:8]} PE {p}"
        assert np.all(bufs[p][DST][total:] == 0xA5)


@pytest.mark.parametrize("P", [1, 2, 3, 5, 8, 17, 64])
def test_collectv_plans(P):
    for name, lens in length_vectors(P).items():
        simulate(P, lens)


def test_collectv_plan_shape():
    """Round 0 the own copy to the exclusive prefix, round 1 send/receive per peer in
    fcollect's order (me + k) % P; a zero length drops its copy and its transfers."""
    lens = [5, 0, 300, 1]
    off = [0, 5, 5, 305]
    for me in range(4):
        pl = S.plan_collect(4, me, lens)
        rounds = pl["rounds"]
        if lens[me]:
            assert [(o["out"], o["ins"], o["count"]) for o in rounds[0]["ops"]] == \
                [((DST, off[me]), [(SRC, 0)], lens[me])] and not rounds[0]["xfers"]
            rounds = rounds[1:]
        (ag,) = rounds
        want = []
        for k in range(1, 4):
            peer = (me + k) % 4
            if lens[me]:
                want.append((1, peer, DST, off[me], lens[me]))
            if lens[peer]:
                want.append((0, peer, DST, off[peer], lens[peer]))
        assert [(x["send"], x["peer"], x["buf"], x["off"], x["bytes"]) for x in ag["xfers"]] == want
        assert not ag["ops"]


def test_collectv_plan_limits():
    with pytest.raises(_lib.SosError):
        S.plan_collect(65, 0, [1] * 65)  # more than PLAN_MAX_PE
    with pytest.raises(_lib.SosError):
        S.plan_collect(3, 3, [1] * 3)
    with pytest.raises(_lib.SosError):
        S.plan_collect(2, 0, [(1 << 64) - 1, 2])  # the sum overflows 64 bits
    with pytest.raises(_lib.SosError):
        S.plan(20, 2, 0, 4, 4)  # a collect plan has no (count, ts) form
    L = S.lib()
    assert L.sosx_plan_encode_collect(2, 0, None, None, None, None, 0) == -3
    s, d = ctypes.c_ulonglong(7), ctypes.c_ulonglong(7)
    assert L.sosx_plan_extents(20, 4, 10, 4, ctypes.byref(s), ctypes.byref(d)) == -3


def test_existing_plans_encode_unchanged():
    """The wire words of plans of existing ids, after collect plans were built in this
    process, equal the words encoded before any was."""
    simulate(5, [3, 0, 17, 255, 1])
    for k, before in BEFORE.items():
        assert _raw(*k) == before, k
