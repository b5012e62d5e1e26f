"""GPU: sosx_sync_snapshot (putsignal.hip), the probe of the point-to-point waits: words of
2, 4 and 8 bytes copied from device memory into pinned host memory, one relaxed system-scope
atomic load each.  1, 63, 64, 65 and 1000 words (one wave, its edges, several workgroups),
starting at an odd element offset; the result equals the device words exactly and the bytes
after it in the host buffer are untouched.  Bad arguments return SOSX_ERR_ARG without a
launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = -3
DTYPES = {2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def state(torch_cuda):
    from sos_amd import shmem as S
    S.lib()
    torch = torch_cuda
    words = np.frombuffer(bytearray(np.random.default_rng(0x5A9).bytes(8 * 1100)), dtype=np.uint8)
    host = torch.empty(8 * 1100, dtype=torch.uint8).pin_memory()
    return {"S": S, "torch": torch, "words": words, "dev": torch.from_numpy(words).cuda(), "host": host}


@pytest.mark.parametrize("width", [2, 4, 8])
@pytest.mark.parametrize("nelems", [1, 63, 64, 65, 1000])
def test_snapshot_equals_the_device_words(state, width, nelems):
    S, torch = state["S"], state["torch"]
    for first in (0, 1, 3):   # odd element offsets: 2-byte words off the 4-byte grid
        state["host"].fill_(0xEE)
        rc = S.sosx_sync_snapshot(state["host"].data_ptr(), state["dev"].data_ptr() + first * width, nelems, width, None)
        assert rc == 0
        torch.cuda.synchronize()
        got = state["host"].numpy()
        want = state["words"][first * width:(first + nelems) * width]
        assert np.array_equal(got[:nelems * width].view(DTYPES[width]), want.view(DTYPES[width])), (width, nelems, first)
        assert (got[nelems * width:] == 0xEE).all(), (width, nelems, first)


def test_bad_arguments_are_refused_before_any_launch(state):
    f = state["S"].sosx_sync_snapshot
    h, d = state["host"].data_ptr(), state["dev"].data_ptr()
    assert f(h, d, 4, 3, None) == ERR_ARG and f(h, d, 4, 1, None) == ERR_ARG and f(h, d, 4, 16, None) == ERR_ARG
    assert f(None, d, 4, 4, None) == ERR_ARG and f(h, None, 4, 4, None) == ERR_ARG
    assert f(h, d + 2, 4, 4, None) == ERR_ARG and f(h + 4, d, 4, 8, None) == ERR_ARG
    assert f(h, d, 0, 8, None) == 0   # nothing to copy
