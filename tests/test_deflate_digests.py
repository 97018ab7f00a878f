"""The GPU deflate's bytes, pinned: both modes (ofd_deflate_batch and
ofd_deflate_lz_batch, include/ofd_deflate.h) must emit exactly the streams
recorded in tests/golden/deflate_digests.json, and the four bound / workspace
functions the values recorded there.

The other deflate tests check that a stream inflates back; this one checks that
it is the same stream as before, so a change to the shared stream format code
(header assembly, CRC fold, bit packer, segment head / tail) shows in either
mode.  The inputs are built by explicit arithmetic only (no RNG), small, and
shaped where that code can go wrong:

- two arrays per call with different content;
- sizes 0, 1, 65, 16385 and 2^20 + 16384 + 5 (two segments, a ragged last chunk
  and a ragged last span);
- `filler` (no match at any candidate distance), `plane` (an f64 plane of small
  integers: zero-dominated, with runs that match at E and at 2E) and `skew`
  (byte counts that, with the end of block, are the Fibonacci numbers, spread
  over the array: 18 or more of them put the deepest Huffman leaf past 15
  bits, so the flatten-and-rebuild loop runs at 16385 bytes and above);
- the literal mode, the match mode with E in {1, 2, 4, 8} at the default
  candidate set, and E = 8 with the candidate set {E} alone.

The fixture is recorded from the library of the commit before a change, never
from the code under test:

    OFD_FW_LIB=<that commit's library> python tests/test_deflate_digests.py
"""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_digests.json")
SEG = 1 << 20
SIZES = (0, 1, 65, 16385, SEG + 16384 + 5)
KINDS = ("filler", "plane", "skew")
# (name, match mode, elem_bytes, candidate mask)
MODES = (("literal", False, 0, 3), ("lz1", True, 1, 3), ("lz2", True, 2, 3), ("lz4", True, 4, 3), ("lz8", True, 8, 3),
         ("lz8_cand0", True, 8, 0))
SIZING = ((0, 0), (1, 0), (0, 5), (1, 1), (2, 65), (2, 16384), (2, 16385), (1, SEG), (3, SEG + 1), (2, SEG + 16384 + 5),
          (64, 8 * 768 * 1024 * 8))


def _lib():
    from opticalflowfromdepth_amd import _native
    return _native.lib()


# ---------------------------------------------------------------- inputs
def _filler(n, i):
    """b[p] = (97 p) & 255 from another start per array: differs from b[p - D] for every D <= 16."""
    return ((97 * (np.arange(n, dtype=np.int64) + 1000 * i)) & 255).astype(np.uint8)


def _plane(n, i):
    """The first n bytes of an f64 plane of integers 0..10, in blocks of 6
    elements: constant (a match at E = 8), alternating with 0 (a match at 2E
    only), or irregular."""
    j = np.arange(n // 8 + 1, dtype=np.int64)
    blk = j // 6 + i
    v = np.where(blk % 3 == 0, blk % 7, np.where(blk % 3 == 1, (j & 1) * (blk % 5 + 1), (j * j + 3 * i) % 11))
    return np.frombuffer(v.astype(np.float64).tobytes(), np.uint8)[:n].copy()


def _skew(n, i):
    """Byte 40 + i + k occurs 1, 2, 3, 5, 8, ... times, for as many k as fit in
    n (in the first segment), one more byte value fills the rest.  With the
    end of block's one occurrence the counts are the Fibonacci numbers 1, 1,
    2, 3, 5, ...: the sum of the first k stays below the next but one, so the
    Huffman tree is a chain whatever way ties are broken, one level per count.
    Position q of that sorted list goes to (q * m) % first, m coprime to
    first = min(n, 1 MiB): the first segment is spread inside itself, so its
    histogram stays."""
    first = min(n, SEG)
    fib, total = [], 0
    a, b = 1, 2
    while total + a <= first and len(fib) < 28:
        fib.append(a)
        total += a
        a, b = b, a + b
    parts = [np.full(f, 40 + i + k, np.uint8) for k, f in enumerate(fib)]
    parts.append(np.full(n - total, 40 + i + len(fib), np.uint8))
    srt = np.concatenate(parts)
    if n < 2:
        return srt
    m = next(p for p in (7919, 104729) if first % p)
    q = np.arange(n, dtype=np.int64)
    out = np.empty(n, np.uint8)
    out[np.where(q < first, (q * m) % first, q)] = srt
    return out


_MAKE = {"filler": _filler, "plane": _plane, "skew": _skew}


def _inputs(kind, n):
    return np.stack([_MAKE[kind](n, i) for i in (0, 1)]).reshape(2, n)


def test_inputs_are_what_the_cases_need():
    """The properties the digest cases rely on, checked on the host."""
    for n in SIZES:
        for kind in KINDS:
            a = _inputs(kind, n)
            assert a.shape == (2, n) and a.dtype == np.uint8
            assert n < 8 or not np.array_equal(a[0], a[1])  # (the first byte of every small f64 integer is 0)
    n = SIZES[-1]
    f = _inputs("filler", n)[0]
    assert all((f[d:] != f[:-d]).all() for d in (1, 2, 4, 8, 16))
    p = _inputs("plane", n)[0]
    assert (p == 0).mean() > 0.75
    e8, e16 = p[8:] == p[:-8], p[16:] == p[:-16]
    # 24 bytes in a row equal to the byte 8 before them; and 24 equal at distance 16 that are not at distance 8

    def run24(m):
        return np.convolve(m.astype(np.int64), np.ones(24, np.int64), "valid") == 24

    r8, r16 = run24(e8[8:]), run24(e16)  # both indexed by position - 16
    assert r8.any() and (r16 & ~r8).any()
    for size in (16385, n):
        s = _inputs("skew", size)[0]
        counts = np.bincount(s[:SEG], minlength=256)
        assert _huffman_depth([int(c) for c in counts if c] + [1]) > 15  # + the end of block


def _huffman_depth(freqs):
    """The longest code of an unrestricted Huffman code over freqs."""
    import heapq
    heap = [(f, 0) for f in freqs]
    heapq.heapify(heap)
    while len(heap) > 1:
        (fa, da), (fb, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (fa + fb, max(da, db) + 1))
    return heap[0][1]


# ---------------------------------------------------------------- CPU: sizing
def _sizing(lib):
    return {f"{c},{b}": [lib.ofd_deflate_bound(b), lib.ofd_deflate_lz_bound(b), lib.ofd_deflate_workspace_bytes(c, b),
                         lib.ofd_deflate_lz_workspace_bytes(c, b)] for c, b in SIZING}


def test_bound_and_workspace_values_are_pinned():
    """ofd_deflate_bound, ofd_deflate_lz_bound, ofd_deflate_workspace_bytes and
    ofd_deflate_lz_workspace_bytes per "count,bytes_each": callers size their
    buffers from them."""
    with open(FIXTURE) as f:
        want = json.load(f)["sizing"]
    assert set(want) == {f"{c},{b}" for c, b in SIZING}
    assert _sizing(_lib()) == want


# ---------------------------------------------------------------- GPU: streams
def _deflate(lib, x, lz, elem):
    """x: device tensor [count, n] uint8 -> (streams, crcs) of one call."""
    import torch
    count, each = x.shape
    bound = (lib.ofd_deflate_lz_bound if lz else lib.ofd_deflate_bound)(each)
    nws = (lib.ofd_deflate_lz_workspace_bytes if lz else lib.ofd_deflate_workspace_bytes)(count, each)
    out = torch.empty(count * bound, dtype=torch.uint8, device=x.device)
    sizes = torch.empty(count, dtype=torch.int64, device=x.device)
    crcs = torch.empty(count, dtype=torch.int32, device=x.device)
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=x.device)
    tail = (out.data_ptr(), sizes.data_ptr(), crcs.data_ptr(), ws.data_ptr(), nws,
            torch.cuda.current_stream().cuda_stream)
    if lz:
        rc = lib.ofd_deflate_lz_batch(x.data_ptr(), count, each, elem, *tail)
    else:
        rc = lib.ofd_deflate_batch(x.data_ptr(), count, each, *tail)
    assert rc == 0
    torch.cuda.synchronize()
    sz = sizes.cpu().tolist()
    assert all(2 <= n <= bound for n in sz)
    host = out.cpu().numpy()
    return ([host[i * bound:i * bound + sz[i]].tobytes() for i in range(count)],
            [int(c) & 0xFFFFFFFF for c in crcs.cpu().tolist()])


def _streams(lib, dev):
    """Every case's record: {"kind/size/mode": {"sizes", "crcs", "sha256"}}."""
    import torch
    got = {}
    for kind in KINDS:
        for n in SIZES:
            a = _inputs(kind, n)
            x = torch.from_numpy(a).to(dev)
            for mode, lz, elem, cand in MODES:
                assert lib.ofd_deflate_lz_set_candidates(cand) == 0
                try:
                    streams, crcs = _deflate(lib, x, lz, elem)
                finally:
                    assert lib.ofd_deflate_lz_set_candidates(3) == 0
                for s, c, row in zip(streams, crcs, a):
                    assert zlib.decompress(s, -15) == row.tobytes() and c == zlib.crc32(row.tobytes()), (kind, n, mode)
                got[f"{kind}/{n}/{mode}"] = {"sizes": [len(s) for s in streams], "crcs": crcs,
                                             "sha256": [hashlib.sha256(s).hexdigest() for s in streams]}
    return got


@pytest.mark.gpu
def test_streams_equal_the_recorded_digests(cuda_device):
    with open(FIXTURE) as f:
        want = json.load(f)["streams"]
    got = _streams(_lib(), cuda_device)
    assert set(got) == set(want) and len(want) == len(KINDS) * len(SIZES) * len(MODES)
    wrong = [k for k in sorted(want) if got[k] != want[k]]
    assert not wrong, wrong
    # the match mode really coded matches on the plane, and none on the filler
    big = SIZES[-1]
    assert want[f"plane/{big}/lz8"]["sizes"][0] < want[f"plane/{big}/literal"]["sizes"][0] // 2
    assert want[f"filler/{big}/lz8"]["sha256"] == want[f"filler/{big}/literal"]["sha256"]


def _record():
    """Write the fixture from the loaded library (OFD_FW_LIB: the parent commit's build)."""
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from opticalflowfromdepth_amd import _native
    lib = _native.lib()
    doc = {"recorded_from_build_id": _native.build_id(), "sizing": _sizing(lib),
           "streams": _streams(lib, torch.device("cuda:0"))}
    path = os.environ.get("OFD_DIGESTS_OUT", FIXTURE)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(doc["streams"]), "stream cases and", len(doc["sizing"]), "sizing rows from build",
          doc["recorded_from_build_id"], "->", path)


if __name__ == "__main__":
    _record()
