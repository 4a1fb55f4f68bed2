"""Every refusal of the four t-SNE entry points, in the order include/ba3c.h states: null pointers,
n or d, the perplexity, lr and momentum, alignment.  A refusal returns before any launch and the
pointers are host addresses that are never dereferenced, so none of this needs a GPU."""
import ctypes

import pytest

BUF = (ctypes.c_int32 * 64)()
BASE = ctypes.addressof(BUF) + -ctypes.addressof(BUF) % 16
NAN, INF = float("nan"), float("inf")
# the arguments after the stream ("+N": the aligned buffer + N bytes) and the keyword of the refusal;
# within an entry point every case also commits the faults of the classes after its own
SQDIST = [((None, 7, 0, "+0", "+4"), b"null"), (("+0", 7, 0, None, "+4"), b"null"), (("+0", 7, 0, "+4", None), b"null"),
          (("+0", 7, 0, "+4", "+0"), b"n must"), (("+0", 8193, 5, "+0", "+0"), b"n must"),
          (("+0", 8, 0, "+4", "+0"), b"d must"), (("+0", 8, 2049, "+0", "+0"), b"d must"),
          (("+4", 8, 5, "+0", "+0"), b"aligned"), (("+0", 8, 5, "+8", "+0"), b"aligned"),
          (("+0", 8, 5, "+0", "+4"), b"aligned")]
AFFIN = [((None, 7, NAN, "+0", "+0", "+4"), b"null"), (("+0", 7, NAN, None, "+0", "+4"), b"null"),
         (("+0", 7, NAN, "+0", None, "+4"), b"null"), (("+0", 7, NAN, "+0", "+0", None), b"null"),
         (("+0", 7, NAN, "+0", "+0", "+4"), b"n must"), (("+0", 8193, NAN, "+0", "+0", "+4"), b"n must"),
         (("+0", 31, NAN, "+0", "+0", "+4"), b"perplexity"), (("+0", 31, INF, "+0", "+0", "+4"), b"perplexity"),
         (("+0", 31, 0.5, "+0", "+0", "+4"), b"perplexity"), (("+0", 31, 10.5, "+0", "+0", "+4"), b"perplexity"),
         (("+4", 31, 10.0, "+0", "+0", "+0"), b"aligned"), (("+0", 31, 10.0, "+4", "+0", "+0"), b"aligned"),
         (("+0", 31, 10.0, "+0", "+8", "+0"), b"aligned"), (("+0", 31, 1.0, "+0", "+0", "+4"), b"aligned")]
# (p, n, y, vel, gains, exag, momentum, lr, work, kl_out)
STEP = [((None, 7, "+0", "+0", "+0", 1.0, 1.0, 0.0, "+4", None), b"null"),
        (("+0", 7, None, "+0", "+0", 1.0, 1.0, 0.0, "+4", None), b"null"),
        (("+0", 7, "+0", None, "+0", 1.0, 1.0, 0.0, "+4", None), b"null"),
        (("+0", 7, "+0", "+0", None, 1.0, 1.0, 0.0, "+4", None), b"null"),
        (("+0", 7, "+0", "+0", "+0", 1.0, 1.0, 0.0, None, None), b"null"),
        (("+0", 7, "+0", "+0", "+0", 1.0, 1.0, 0.0, "+4", None), b"n must"),
        (("+0", 8193, "+0", "+0", "+0", 1.0, 1.0, 0.0, "+4", None), b"n must"),
        (("+0", 8, "+0", "+0", "+0", 1.0, 1.0, 0.0, "+4", None), b"lr"),
        (("+0", 8, "+0", "+0", "+0", 1.0, 1.0, NAN, "+4", None), b"lr"),
        (("+0", 8, "+0", "+0", "+0", 1.0, 1.0, INF, "+4", None), b"lr"),
        (("+0", 8, "+0", "+0", "+0", 1.0, 1.0, 200.0, "+4", None), b"momentum"),
        (("+0", 8, "+0", "+0", "+0", 1.0, -0.1, 200.0, "+4", None), b"momentum"),
        (("+0", 8, "+0", "+0", "+0", 1.0, NAN, 200.0, "+4", None), b"momentum"),
        (("+4", 8, "+0", "+0", "+0", 1.0, 0.5, 200.0, "+0", None), b"aligned"),
        (("+0", 8, "+8", "+0", "+0", 1.0, 0.5, 200.0, "+0", None), b"aligned"),
        (("+0", 8, "+0", "+4", "+0", 1.0, 0.5, 200.0, "+0", None), b"aligned"),
        (("+0", 8, "+0", "+0", "+8", 1.0, 0.5, 200.0, "+0", None), b"aligned"),
        (("+0", 8, "+0", "+0", "+0", 1.0, 0.5, 200.0, "+4", None), b"aligned"),
        (("+0", 8, "+0", "+0", "+0", 1.0, 0.5, 200.0, "+0", "+4"), b"aligned")]
CASES = ([("ba3c_tsne_sqdist",) + c for c in SQDIST] + [("ba3c_tsne_affinities",) + c for c in AFFIN] +
         [("ba3c_tsne_step",) + c for c in STEP])


@pytest.mark.parametrize("entry,args,word", CASES)
def test_refusals_in_the_stated_order(entry, args, word):
    from ba3c_amd import _lib as L
    lib = L.load()
    args = [ctypes.c_void_p(BASE + int(a)) if isinstance(a, str) else a for a in args]
    assert getattr(lib, entry)(None, *args) == 1
    assert word in lib.ba3c_last_error(), lib.ba3c_last_error()


def test_the_workspace_size():
    from ba3c_amd import _lib as L
    lib = L.load()
    for n, d in ((7, 5), (8193, 5), (8, 0), (8, 2049)):
        assert lib.ba3c_tsne_workspace_size(n, d) == 0
    small, big = lib.ba3c_tsne_workspace_size(8192, 1), lib.ba3c_tsne_workspace_size(8192, 2048)
    assert small >= 8192 * (4 + 4 + 48) and big - small >= 8192 * 2047 * 4 and big % 256 == 0
