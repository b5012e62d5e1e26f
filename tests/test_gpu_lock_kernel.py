"""GPU: sosx_lock_step (lock.hip) in one process.  P = 4 PEs are emulated as four 8-byte lock
words in one device buffer with 64 B of canary on both sides; the table points at the four
words.  The scripts of tests/lock_proto_harness.cpp are driven through the kernel: an
uncontended acquire and release, the queue 0, 2, 1 released in turn, try on a held lock, a
release that finds its successor not yet linked (PENDING, nothing changed) and the later
hand-off, and the final all-zero state.  After EVERY launch all four words, the result record
and both canaries are compared with a model of the queue kept here (a list of PE ids).  The
out-of-range values are the CPU harness's: no launch here is given a garbage lock."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 4
GUARD = 64
CANARY = 0xA5
ENQUEUE, TRY, RELEASE, HANDOFF = range(4)
ACQUIRED, QUEUED, BUSY, RELEASED, HANDED, PENDING, CORRUPT = range(7)
SIGNAL = 0x80000000


class Model:
    """Who is queued (front = holder), who has linked itself, who was granted by a hand-off."""

    def __init__(self):
        self.queue, self.linked, self.signalled = [], {}, {}

    def last(self):
        return self.queue[-1] + 1 if self.queue else 0

    def data(self, q):
        if q not in self.queue:
            return 0
        i = self.queue.index(q)
        v = SIGNAL if self.signalled[q] else 0
        if i + 1 < len(self.queue) and self.linked[self.queue[i + 1]]:
            v |= self.queue[i + 1] + 1
        return v

    def join(self, q, linked=True):
        self.queue.append(q)
        self.linked[q], self.signalled[q] = linked, False

    def leave(self):
        self.queue.pop(0)
        if self.queue:
            self.signalled[self.queue[0]] = True

    def words(self):
        return [(self.last() if q == 0 else 0) | (self.data(q) << 32) for q in range(P)]


@pytest.fixture(scope="module")
def arena(torch_cuda):
    from sos_amd import shmem as S
    S.lib()
    torch = torch_cuda
    buf = torch.empty(GUARD + 8 * P + GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 8 == 0
    base = buf.data_ptr() + GUARD
    table = torch.tensor([base + 8 * q for q in range(P)], dtype=torch.int64, device="cuda")
    record = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return {"S": S, "torch": torch, "buf": buf, "base": base, "table": table, "record": record, "launches": 0}


def reset(a, model):
    a["buf"].fill_(CANARY)
    a["buf"][GUARD:GUARD + 8 * P] = 0
    a["torch"].cuda.synchronize()
    verify(a, model, "a zeroed lock")


def verify(a, model, what):
    host = a["buf"].cpu().numpy()
    assert (host[:GUARD] == CANARY).all() and (host[GUARD + 8 * P:] == CANARY).all(), f"{what}: a canary changed"
    got = [int(w) for w in host[GUARD:GUARD + 8 * P].view(np.uint64)]
    assert got == model.words(), f"{what}: words {[hex(w) for w in got]}, model {[hex(w) for w in model.words()]}"


def step(a, kind, me, model, what, status, prev, data=0):
    S, torch = a["S"], a["torch"]
    a["record"].fill_(-1)
    rc = S.sosx_lock_step(kind, a["base"], a["base"] + 8 * me + 4, a["table"].data_ptr(), 4, me, P,
                          a["record"].data_ptr(), None)
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    a["launches"] += 1
    rec = a["record"].cpu().numpy()
    got = (int(rec[0]), int(rec[1]) & 0xFFFFFFFF, int(rec[2]), int(rec[3]))
    assert got == (prev, data, status, 0), f"{what}: record (prev, data, status, bad) = {got}"
    verify(a, model, what)


def test_uncontended(arena):
    for me in range(P):
        m = Model()
        reset(arena, m)
        m.join(me)
        step(arena, ENQUEUE, me, m, f"PE {me} enqueues on a free lock", ACQUIRED, 0)
        m.leave()
        step(arena, RELEASE, me, m, f"PE {me} releases", RELEASED, me + 1)
        m.join(me)
        step(arena, TRY, me, m, f"PE {me} tries a free lock", ACQUIRED, 0)
        m.leave()
        step(arena, RELEASE, me, m, f"PE {me} releases after try", RELEASED, me + 1)
        assert m.words() == [0] * P


def test_queue_0_2_1_released_in_turn(arena):
    m = Model()
    reset(arena, m)
    m.join(0)
    step(arena, ENQUEUE, 0, m, "PE 0 enqueues", ACQUIRED, 0)
    m.join(2)
    step(arena, ENQUEUE, 2, m, "PE 2 enqueues behind 0", QUEUED, 1)
    m.join(1)
    step(arena, ENQUEUE, 1, m, "PE 1 enqueues behind 2", QUEUED, 3)
    m.leave()
    step(arena, RELEASE, 0, m, "PE 0 hands over to 2", HANDED, 2, data=3)
    assert m.data(2) == SIGNAL | 2 and m.data(1) == 0
    m.leave()
    step(arena, RELEASE, 2, m, "PE 2 hands over to 1", HANDED, 2, data=SIGNAL | 2)
    m.leave()
    step(arena, RELEASE, 1, m, "PE 1 releases", RELEASED, 2)
    assert m.words() == [0] * P


def test_try_on_a_held_lock_touches_only_own_data(arena):
    m = Model()
    reset(arena, m)
    m.join(1)
    step(arena, ENQUEUE, 1, m, "PE 1 enqueues", ACQUIRED, 0)
    # stale bits in PE 3's data half: its try zeroes them, and nothing else changes
    arena["buf"][GUARD + 8 * 3 + 4] = 0x34
    arena["torch"].cuda.synchronize()
    step(arena, TRY, 3, m, "PE 3 tries the held lock", BUSY, 2)
    step(arena, TRY, 0, m, "PE 0 tries the held lock", BUSY, 2)
    m.leave()
    step(arena, RELEASE, 1, m, "PE 1 releases", RELEASED, 2)
    assert m.words() == [0] * P


def test_pending_release_then_the_hand_off(arena):
    torch = arena["torch"]
    m = Model()
    reset(arena, m)
    m.join(3)
    step(arena, ENQUEUE, 3, m, "PE 3 enqueues", ACQUIRED, 0)
    # PE 1's enqueue stopped between its swap and its link: last = 2, its data zero
    words = arena["buf"][GUARD:GUARD + 8 * P].view(torch.int32)
    words[0] = 2
    torch.cuda.synchronize()
    m.join(1, linked=False)
    verify(arena, m, "PE 1 swapped but not linked")
    step(arena, RELEASE, 3, m, "PE 3 releases before the link", PENDING, 2)
    step(arena, HANDOFF, 3, m, "PE 3's hand-off before the link", PENDING, 0)
    # the rest of PE 1's enqueue: NEXT into PE 3's data
    words[2 * 3 + 1] = 2
    torch.cuda.synchronize()
    m.linked[1] = True
    verify(arena, m, "PE 1 linked")
    m.leave()
    step(arena, HANDOFF, 3, m, "PE 3's later hand-off", HANDED, 0, data=2)
    m.leave()
    step(arena, RELEASE, 1, m, "PE 1 releases", RELEASED, 2)
    assert m.words() == [0] * P
