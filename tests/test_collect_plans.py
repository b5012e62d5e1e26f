"""CPU: the fcollect and alltoall plans of every PE, decoded through the C ABI and run by a
small byte-buffer simulator (transfers matched FIFO per (sender, receiver) pair, as RCCL
matches ncclSend/ncclRecv), against the closed forms of SOS's index arithmetic
(src/collectives.c:1284-1480):

  fcollect:  target of every PE = concat over q of source(q)            (my_as_rank * len)
  alltoall:  target(i) block j  = source(j) block i                     (peer_as_rank * len)
"""
import numpy as np
import pytest

from sos_amd import _lib
from sos_amd import shmem as S

SRC, DST, SCR = 0, 1, 2
COPY = 1
IDS = {"fcollect": 18, "alltoall": 19}


def sources(alg, P, B):
    """Per-PE source bytes: fcollect B bytes, alltoall P blocks of B bytes."""
    n = B if alg == "fcollect" else P * B
    return [np.random.default_rng(1000 * P + q).integers(0, 256, n, dtype=np.uint8) for q in range(P)]


def expected(alg, P, B, srcs):
    if alg == "fcollect":
        return [np.concatenate(srcs)] * P
    return [np.concatenate([srcs[j][i * B:(i + 1) * B] for j in range(P)]) for i in range(P)]


def simulate(alg, P, count, ts, mis):
    B = count * ts
    sb, db = _lib.plan_extents(alg, P, count, ts)
    plans = [S.plan(IDS[alg], P, p, count, ts, mis[0], mis[1]) for p in range(P)]
    srcs = sources(alg, P, B)
    assert all(s.size == sb for s in srcs)
    bufs = [{SRC: srcs[p], DST: np.full(db, 0xA5, dtype=np.uint8)} for p in range(P)]
    extent = {SRC: sb, DST: db}
    written = [np.zeros(db, dtype=bool) for _ in range(P)]
    nsend = nrecv = 0
    for p, pl in enumerate(plans):
        assert pl["alg"] == IDS[alg] and pl["scratch_bytes"] == 0
        for r in pl["rounds"]:
            for x in r["xfers"]:
                assert x["bytes"] > 0, "empty transfer"
                assert x["buf"] in (SRC, DST) and 0 <= x["peer"] < P and x["peer"] != p
                assert 0 <= x["off"] and x["off"] + x["bytes"] <= extent[x["buf"]], (p, x)
                assert x["send"] or x["buf"] == DST
                nsend += x["send"]
                nrecv += 1 - x["send"]
            for l in r["ops"]:
                assert l["kind"] == COPY and len(l["ins"]) == 1 and l["count"] > 0
                (ib, ioff), (ob, ooff) = l["ins"][0], l["out"]
                assert ob == DST and ooff + l["count"] <= db
                assert ib in (SRC, DST) and ioff + l["count"] <= extent[ib]
    assert nsend == nrecv
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
                if any(not y["send"] and y["peer"] == x["peer"] and not done[p][j]
                       for j, y in enumerate(r["xfers"][:i])):
                    ok = False
                    continue
                q = fifo.get((x["peer"], p), [])
                if not q:
                    ok = False
                    continue
                data = q.pop(0)
                assert data.size == x["bytes"], "plan size mismatch between PEs"
                bufs[p][DST][x["off"]:x["off"] + x["bytes"]] = data
                written[p][x["off"]:x["off"] + x["bytes"]] = True
                outstanding[x["peer"]] -= 1
                done[p][i] = True
                progress = True
            if ok and outstanding[p] == 0:
                for l in r["ops"]:
                    (ib, ioff), (ob, ooff), n = l["ins"][0], l["out"], l["count"]
                    bufs[p][ob][ooff:ooff + n] = bufs[p][ib][ioff:ioff + n].copy()
                    written[p][ooff:ooff + n] = True
                k[p] += 1
                posted[p] = False
                progress = True
        if all_done:
            break
        assert progress, "plans deadlock"
    assert not any(fifo.values()), "unmatched sends"
    exp = expected(alg, P, B, srcs)
    for p in range(P):
        assert written[p].all(), f"PE {p}: target bytes never written"
        assert np.array_equal(bufs[p][DST], exp[p]), f"{alg} P={P} count={count} ts={ts} PE {p}"


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 8, 9, 12, 16, 64])
@pytest.mark.parametrize("alg", ["fcollect", "alltoall"])
def test_collect_plans(alg, P):
    for count in (1, 3, 4099):
        for ts in (1, 4, 16):
            for mis in ((0, 0), (4, 12)):
                simulate(alg, P, count, ts, mis)


@pytest.mark.parametrize("alg", ["fcollect", "alltoall"])
def test_collect_plan_shapes(alg):
    """fcollect: the own copy, then one direct allgather round inside DST (the shape the
    RCCL executor hands to ncclAllGather); alltoall: one exchange round, then the self block."""
    P, n, ts = 5, 7, 4
    B = n * ts
    for me in range(P):
        pl = S.plan(IDS[alg], P, me, n, ts)
        if alg == "fcollect":
            assert len(pl["rounds"]) == 2
            c, ag = pl["rounds"]
            assert not c["xfers"] and [(o["out"], o["ins"], o["count"]) for o in c["ops"]] == \
                [((DST, me * B), [(SRC, 0)], B)]
            assert not ag["ops"] and len(ag["xfers"]) == 2 * (P - 1)
            for x in ag["xfers"]:
                owner = me if x["send"] else x["peer"]
                assert (x["buf"], x["off"], x["bytes"]) == (DST, owner * B, B)
        else:
            assert len(pl["rounds"]) == 1
            r = pl["rounds"][0]
            assert len(r["xfers"]) == 2 * (P - 1)
            for x in r["xfers"]:
                assert (x["buf"], x["off"], x["bytes"]) == (SRC if x["send"] else DST, x["peer"] * B, B)
            assert [(o["out"], o["ins"], o["count"]) for o in r["ops"]] == [((DST, me * B), [(SRC, me * B)], B)]


@pytest.mark.parametrize("alg", ["fcollect", "alltoall"])
def test_collect_plan_count_zero_and_limits(alg):
    for P in (1, 3, 64):
        assert S.plan(IDS[alg], P, 0, 0, 4)["rounds"] == []
    with pytest.raises(_lib.SosError):
        S.plan(IDS[alg], 65, 0, 4, 4)  # more than PLAN_MAX_PE
    with pytest.raises(_lib.SosError):
        S.plan(9, 4, 0, 4, 4)  # id 9 stays invalid
