"""The match mode of the GPU deflate (ofd_deflate_lz_batch, include/ofd_deflate.h)
and the writer on top of it (GpuNpzWriter(matches=True), --writer gpu-lz).

The checker is host zlib: every stream inflates (zlib.decompress(s, -15)) to
exactly the array's bytes and carries zlib's CRC-32.  The encoder parses each
64-byte span greedily for runs b[p+i] == b[p+i-D], D in {1, E, 2E} (E = the
element size), minimum length 3, so matches are 3..64 bytes long.
"""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

from opticalflowfromdepth_amd import preprocess as pp

SEG = 1 << 20
EINVAL, EWORKSPACE, EALIGN = -1, -3, -4


def _lib():
    from opticalflowfromdepth_amd import _native
    return _native.lib()


# ---------------------------------------------------------------- CPU
def test_lz_argument_errors_without_gpu():
    """Validation happens before any HIP call."""
    lib = _lib()
    f = lib.ofd_deflate_lz_batch
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)  # never dereferenced
    ws = lib.ofd_deflate_lz_workspace_bytes(2, 100000)
    assert ws > 0 and lib.ofd_deflate_lz_workspace_bytes(0, 100) == 0 and lib.ofd_deflate_lz_workspace_bytes(3, 0) == 0
    for e in (0, 3, 5, 16, -1):
        assert f(p, 2, 100000, e, p, p, p, p, ws, None) == EINVAL
    assert f(p, -1, 100, 8, p, p, p, p, ws, None) == EINVAL
    assert f(p, 1, -100, 8, p, p, p, p, ws, None) == EINVAL
    assert f(None, 2, 100000, 8, p, p, p, p, ws, None) == EINVAL
    assert f(p, 2, 100000, 8, None, p, p, p, ws, None) == EINVAL
    assert f(p, 2, 100000, 8, p, None, p, p, ws, None) == EINVAL
    assert f(p, 2, 100000, 8, p, p, None, p, ws, None) == EINVAL
    assert f(p, 2, 100000, 8, q, p, p, p, ws, None) == EALIGN
    assert f(p, 2, 100000, 8, p, p, p, p, ws - 1, None) == EWORKSPACE
    assert f(p, 2, 100000, 8, p, p, p, None, ws, None) == EWORKSPACE
    assert f(None, 0, 100000, 8, None, None, None, None, 0, None) == 0  # count == 0: nothing to do
    assert lib.ofd_deflate_lz_set_candidates(4) == EINVAL and lib.ofd_deflate_lz_set_candidates(3) == 0


def test_lz_bound_covers_the_worst_case():
    """<= 15 bits per input byte (a literal; a match is <= 37 bits for >= 3
    bytes), per segment a header of <= 14 + 57 + 316 * 7 bits, the 15-bit end
    of block and the sync marker (3 bits, padding, 4 bytes), then 2 bytes."""
    lib = _lib()
    for n in (0, 1, 63, 16384, SEG - 1, SEG, SEG + 1, 8 * 768 * 1024 * 8, 44 * 768 * 1024 * 8):
        segs = (n + SEG - 1) // SEG
        worst = (15 * n + segs * (14 + 57 + 316 * 7 + 15 + 3 + 7)) // 8 + segs * 5 + 2
        b = lib.ofd_deflate_lz_bound(n)
        assert b % 256 == 0 and b >= worst, n


def test_make_writer_gpu_lz():
    w = pp.make_writer("gpu-lz")
    try:
        assert type(w).__name__ == "GpuNpzWriter" and w.matches is True
    finally:
        w.close()
    w = pp.make_writer("gpu")
    assert w.matches is False
    w.close()


def test_cli_accepts_writer_gpu_lz():
    # argparse checks --writer's choice before it reaches --help (exit 0); an unknown choice exits 2
    with pytest.raises(SystemExit) as e:
        pp.main(["--writer", "gpu-lz", "--help"])
    assert e.value.code == 0
    with pytest.raises(SystemExit) as e:
        pp.main(["--writer", "gpu-lzz", "--help"])
    assert e.value.code == 2


def test_stream_reader_on_zlib_output():
    """The tests' own token reader (_matches), checked on zlib's streams."""
    data = bytes(range(7)) * 50
    for level in (1, 9):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        m = _matches(c.compress(data) + c.flush())
        assert m and all(d % 7 == 0 and 3 <= ln <= 258 for ln, d in m)
        # all but the first period (and a literal or two of zlib's lazy evaluation) is matched
        assert len(data) - 10 <= sum(ln for ln, _ in m) <= len(data) - 7


# ---------------------------------------------------------------- GPU
def _run(x, elem=None, lz=True, ws=None, stream=None):
    """x: device tensor [count, ...] -> (streams, crcs, bound) of one call."""
    lib = _lib()
    count = x.shape[0]
    each = int(x[0].numel() * x.element_size()) if count else 0
    elem = elem or x.element_size()
    bound = (lib.ofd_deflate_lz_bound if lz else lib.ofd_deflate_bound)(each)
    out = torch.empty(max(count * bound, 1), dtype=torch.uint8, device=x.device)
    sizes = torch.empty(max(count, 1), dtype=torch.int64, device=x.device)
    crcs = torch.empty(max(count, 1), dtype=torch.int32, device=x.device)
    nws = (lib.ofd_deflate_lz_workspace_bytes if lz else lib.ofd_deflate_workspace_bytes)(count, each)
    if ws is None:
        ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=x.device)
    assert ws.numel() >= nws
    st = (stream or torch.cuda.current_stream()).cuda_stream
    tail = (out.data_ptr(), sizes.data_ptr(), crcs.data_ptr(), ws.data_ptr(), ws.numel(), st)
    if lz:
        rc = lib.ofd_deflate_lz_batch(x.data_ptr(), count, each, elem, *tail)
    else:
        rc = lib.ofd_deflate_batch(x.data_ptr(), count, each, *tail)
    assert rc == 0
    torch.cuda.synchronize()
    sz = sizes.cpu().tolist()[:count]
    assert all(2 <= n <= bound for n in sz)
    streams = [bytes(out[i * bound:i * bound + sz[i]].cpu().numpy()) for i in range(count)]
    return streams, [int(c) & 0xFFFFFFFF for c in crcs.cpu().tolist()[:count]]


def _check(streams, crcs, arrays):
    """arrays: per stream, the bytes it must inflate to."""
    assert len(streams) == len(arrays)
    for i, (s, c, a) in enumerate(zip(streams, crcs, arrays)):
        raw = zlib.decompress(s, -15)
        assert raw == a, i
        assert c == zlib.crc32(a), i


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
          6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def _matches(s):
    """A minimal RFC 1951 reader (tests' own, for small streams): the
    (length, distance) of every match in the raw-deflate stream s, in order."""
    pos = 0

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((s[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v

    def table(lens):  # canonical Huffman codes: (length, code) -> symbol
        tab, code = {}, 0
        for ln in range(1, 16):
            for sy, l in enumerate(lens):
                if l == ln:
                    tab[(ln, code)] = sy
                    code += 1
            code <<= 1
        return tab

    def sym(tab):
        code = ln = 0
        while True:
            code, ln = (code << 1) | bits(1), ln + 1
            assert ln <= 15
            if (ln, code) in tab:
                return tab[(ln, code)]

    out = []
    while True:
        final, btype = bits(1), bits(2)
        if btype == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            assert bits(16) == n ^ 0xFFFF
            pos += 8 * n
        else:
            if btype == 1:
                lt = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
                dt = table([5] * 30)
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][i]] = bits(3)
                ct, lens = table(cl), []
                while len(lens) < hlit + hdist:
                    c = sym(ct)
                    if c < 16:
                        lens.append(c)
                    elif c == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * (3 + bits(3) if c == 17 else 11 + bits(7))
                lt, dt = table(lens[:hlit]), table(lens[hlit:])
            while True:
                c = sym(lt)
                if c == 256:
                    break
                if c > 256:
                    ln = _LBASE[c - 257] + bits(_LEXT[c - 257])
                    d = sym(dt)
                    out.append((ln, _DBASE[d] + bits(_DEXT[d])))
        if final:
            return out


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _filler(n, start=0):
    """b[p] = (97 p) & 255: differs from b[p - D] for every D <= 16."""
    return ((97 * (np.arange(n, dtype=np.int64) + start)) & 255).astype(np.uint8)


def _sizes(E):
    return sorted({0, 1, 2, 3, E - 1, E, E + 1, 63, 64, 65, 16383, 16384, 16385, SEG - 1, SEG, SEG + 1,
                   SEG + 16384 + 5})


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_lz_boundaries_with_matches_everywhere(cuda_device, E, count):
    """Every size around the span (64), chunk (16 KiB) and segment (1 MiB)
    boundaries, with content that wants a match at every byte: one constant
    byte, and a random E-byte pattern repeated."""
    rng = np.random.default_rng(100 * E + count)
    for n in _sizes(E):
        const = np.stack([np.full(n, 7 + i, np.uint8) for i in range(count)])
        pat = np.stack([np.resize(rng.integers(0, 256, E).astype(np.uint8), n) for _ in range(count)])
        for a in (const, pat):
            a = a.reshape(count, n)
            s, c = _run(_dev(a, cuda_device), E)
            _check(s, c, [a[i].tobytes() for i in range(count)])


@pytest.mark.gpu
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_lz_batch_isolation(cuda_device, E):
    """Three identical constant arrays in one call: each stream inflates on its
    own (a match reaching into the previous array would be 'too far back')."""
    n = 70000
    a = np.full((3, n), 0x5A, np.uint8)
    s, c = _run(_dev(a, cuda_device), E)
    _check(s, c, [a[i].tobytes() for i in range(3)])
    assert s[0] == s[1] == s[2]


def _cands(E):
    return sorted({1, E, 2 * E})


@pytest.mark.gpu
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_lz_distance_alphabet(cuda_device, E):
    """One distance code alone (D distinct bytes tiled: the only repeats are at
    multiples of D), a mix of all of them in one block, and no match at all."""
    rng = np.random.default_rng(E)
    n = SEG + 16384 + 5
    for D in _cands(E):
        a = np.resize(rng.permutation(256)[:D].astype(np.uint8), n).reshape(1, n)
        s, c = _run(_dev(a, cuda_device), E)
        _check(s, c, [a.tobytes()])
        assert len(s[0]) < n // 8  # below the floor of any literal-only stream
        assert {d for _, d in _matches(s[0])} == {D}
    # blocks of 200 bytes, each tiled at one of the candidate distances, cycling through them
    parts = []
    for i in range(n // 200 + 1):
        D = _cands(E)[i % len(_cands(E))]
        parts.append(np.resize(rng.permutation(256)[:D].astype(np.uint8), 200))
    mix = np.concatenate(parts)[:n].reshape(1, n)
    s, c = _run(_dev(mix, cuda_device), E)
    _check(s, c, [mix.tobytes()])
    assert len(s[0]) < n // 8
    assert {d for _, d in _matches(s[0])} == set(_cands(E))
    # no match: the literal histogram is the literal encoder's, only the header may grow
    none = _filler(n).reshape(1, n)
    x = _dev(none, cuda_device)
    s, c = _run(x, E)
    _check(s, c, [none.tobytes()])
    lit, _ = _run(x, lz=False)
    assert len(s[0]) <= len(lit[0]) + 64 * 2


@pytest.mark.gpu
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_lz_length_alphabet(cuda_device, E):
    """Every match length 3..64 (all the encoder emits: a match stays in its
    64-byte span), at a span start, for every candidate distance: the D bytes
    before the span and its first L bytes tile D distinct bytes, between
    separators that repeat nowhere.  Both sides of the length-code boundaries
    10/11, 12/13, ... 18/19, 22/23, ... 34/35, 42/43, 50/51, 58/59 are in."""
    rng = np.random.default_rng(10 + E)
    lens = list(range(3, 65))
    arrays = []
    for D in _cands(E):
        b = _filler(128 * (len(lens) + 1))
        for i, L in enumerate(lens):
            p = 128 * i + 64  # a span start with a span of separators before it
            while True:
                pat = rng.permutation(256)[:D].astype(np.uint8)
                # the run ends after L bytes: the separator behind it differs from the byte that would extend it
                if L == 64 or b[p + L] != pat[L % D]:
                    break
            b[p - D:p + L] = np.resize(pat, D + L)
        arrays.append(b)
    a = np.stack(arrays)
    s, c = _run(_dev(a, cuda_device), E)
    _check(s, c, [x.tobytes() for x in arrays])
    for D, st in zip(_cands(E), s):
        got = set(_matches(st))
        assert not {(L, D) for L in lens} - got, (D, sorted({(L, D) for L in lens} - got))


@pytest.mark.gpu
@pytest.mark.parametrize("E", [1, 8])
def test_lz_code_length_limit_and_noise(cuda_device, E):
    """Histograms that force the 15-bit limit on the 286-symbol alphabet (one
    dominant byte with a tail of rare ones; byte counts that grow like the
    Fibonacci numbers, shuffled) and incompressible noise, which must stay
    inside ofd_deflate_lz_bound (checked by _run)."""
    rng = np.random.default_rng(9)
    n = 3 << 20
    skew = np.zeros(n, np.uint8)
    idx = rng.choice(n, 3000, replace=False)
    skew[idx] = rng.integers(1, 256, 3000).astype(np.uint8)
    flat = rng.integers(0, 256, n).astype(np.uint8)
    fib = [1, 1]
    while len(fib) < 28:
        fib.append(fib[-1] + fib[-2])
    first = np.concatenate([np.full(f, 40 + k, np.uint8) for k, f in enumerate(fib)])
    first = np.concatenate([first, np.full(SEG - first.size, 40 + len(fib), np.uint8)])
    rng.shuffle(first)
    deep = np.concatenate([first, flat[:n - SEG]])
    a = np.stack([skew, flat, deep])
    s, c = _run(_dev(a, cuda_device), E)
    _check(s, c, [a[i].tobytes() for i in range(3)])
    assert len(s[0]) < n // 8


@pytest.mark.gpu
def test_lz_matches_are_really_coded(cuda_device):
    """A literal costs at least one bit, so no literal-only stream of n bytes is
    shorter than n / 8: a constant array that deflates below that was coded
    with matches.  (Reached: one 64-byte match per span, about n / 80.)"""
    n = 3 << 20
    a = np.full((1, n), 7, np.uint8)
    x = _dev(a, cuda_device)
    s, c = _run(x, 1)
    _check(s, c, [a.tobytes()])
    print("constant 3 MiB:", len(s[0]), "bytes")
    assert len(s[0]) < n // 8
    lit, _ = _run(x, lz=False)
    assert len(lit[0]) >= n // 8


def _planes(h=96, w=128):
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.round(127.5 + 100 * np.sin(xx / 17.0) * np.cos(yy / 23.0) + 20 * np.sin((xx + yy) / 5.0))
    ints = np.clip(smooth, 0, 255)
    depth = (2.0 + 0.01 * xx + 0.02 * yy + 0.3 * np.sin(xx / 9.0)).astype(np.float32)
    depth[:h // 3] = 100.0  # the constant region (depth == 100)
    mask = ((xx - w / 2) ** 2 + (yy - h / 2) ** 2 < (h / 3) ** 2).astype(np.float64)
    return {"ints": ints, "f32vals": depth.astype(np.float64), "mask": mask}


@pytest.mark.gpu
def test_lz_product_like_planes(cuda_device):
    """f64 planes of integers 0..255, of f32 values with a constant region, a
    0/1 mask, and their f32 versions: never more than 64 bytes per segment
    above the literal encoder's stream; strictly smaller for the integer and
    mask planes."""
    for name, p in _planes().items():
        for dt in (np.float64, np.float32):
            a = p.astype(dt)[None]
            x = _dev(a, cuda_device)
            s, c = _run(x)
            _check(s, c, [a.tobytes()])
            lit, lc = _run(x, lz=False)
            _check(lit, lc, [a.tobytes()])
            segs = (a.nbytes + SEG - 1) // SEG
            print(name, np.dtype(dt).name, "bytes", a.nbytes, "literal", len(lit[0]), "lz", len(s[0]))
            assert len(s[0]) <= len(lit[0]) + 64 * segs, (name, dt)
            if name in ("ints", "mask"):
                assert len(s[0]) < len(lit[0]), (name, dt)


@pytest.mark.gpu
def test_lz_plumbing(cuda_device):
    """An input 3 bytes off 16-byte alignment, a non-default stream, and one
    workspace reused across calls of different sizes."""
    rng = np.random.default_rng(5)
    lib = _lib()
    base = np.repeat(rng.integers(0, 256, 40000).astype(np.uint8), 5)  # runs of 5
    store = _dev(base, cuda_device)
    view = store[3:3 + 2 * 70001].view(2, 70001)
    assert view.data_ptr() % 16 == 3
    want = [base[3:3 + 70001].tobytes(), base[3 + 70001:3 + 2 * 70001].tobytes()]
    ws = torch.empty(lib.ofd_deflate_lz_workspace_bytes(2, SEG + 100) + 256, dtype=torch.uint8, device=cuda_device)
    s, c = _run(view, 1, ws=ws)
    _check(s, c, want)
    st = torch.cuda.Stream(cuda_device)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s2, c2 = _run(view, 1, ws=ws, stream=st)
    assert s2 == s and c2 == c
    big = _dev(np.resize(base, (2, SEG + 100)), cuda_device)
    s, c = _run(big, 4, ws=ws)
    _check(s, c, [bytes(big[i].cpu().numpy()) for i in range(2)])
    small = _dev(np.resize(base, (1, 77)), cuda_device)
    s, c = _run(small, 2, ws=ws)
    _check(s, c, [bytes(small[0].cpu().numpy())])
    s, c = _run(view, 8, ws=ws)
    _check(s, c, want)


@pytest.mark.gpu
def test_lz_writer_files_load_back(cuda_device, tmp_path):
    from opticalflowfromdepth_amd.npz_gpu import GpuNpzWriter
    x = torch.randint(0, 256, (4, 8, 64, 80), device=cuda_device).to(torch.float64)
    x[:, 4:] = torch.randn(4, 4, 64, 80, device=cuda_device).to(torch.float32).to(torch.float64)
    x[:, 7] = (x[:, 7] > 0).to(torch.float64)
    w = GpuNpzWriter(workers=2, matches=True)
    paths = [str(tmp_path / f"{i}_0_1.npz") for i in range(4)]
    w.save_batch(paths, x, "img_depth_flow", {"augment_flow_type": np.array(6)})
    w.save(str(tmp_path / "group.npz"), img_depth_flow=x[1].to(torch.float32))
    w.close()
    xs = x.cpu().numpy()
    for i, p in enumerate(paths):
        z = np.load(p)
        assert sorted(z.files) == ["augment_flow_type", "img_depth_flow"]
        assert z["img_depth_flow"].dtype == np.float64 and np.array_equal(z["img_depth_flow"], xs[i])
        assert int(z["augment_flow_type"]) == 6
    g = np.load(str(tmp_path / "group.npz"))["img_depth_flow"]
    assert g.dtype == np.float32 and np.array_equal(g, xs[1].astype(np.float32))
    assert w.bytes_written > 0 and w.bytes_in == 4 * xs[0].nbytes + xs[1].nbytes // 2


@pytest.mark.gpu
def test_pipeline_files_with_lz_writer_equal_zlib_writer(cuda_device, tmp_path):
    """run_batch writing its 121 files per image through the match-mode writer:
    every array np.load-equal to the same run through the zlib NpzWriter."""
    from opticalflowfromdepth_amd import synth
    from opticalflowfromdepth_amd.npz_gpu import GpuNpzWriter
    seeds = [77, 78]
    h, w = 48, 64
    img0 = synth.synthetic_rgb(seeds, h, w, cuda_device)
    depth = synth.synthetic_depth(seeds, h, w, cuda_device, dtype=torch.float64)
    dirs = {}
    for tag, writer in (("zlib", pp.NpzWriter(4, 1)), ("lz", GpuNpzWriter(4, matches=True))):
        ppa = pp.PreprocessPlusAugment(cuda_device)
        ppa.writer = writer
        dirs[tag] = [str(tmp_path / tag / str(s)) for s in seeds]
        ppa.run_batch(seeds, img0, depth, out_dirs=dirs[tag])
        writer.close()
    for a, b in zip(dirs["zlib"], dirs["lz"]):
        fa = sorted(os.listdir(a))
        assert fa == sorted(os.listdir(b)) and len(fa) == 121
        for f in fa:
            za, zb = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
            assert sorted(za.files) == sorted(zb.files), f
            for k in za.files:
                assert za[k].dtype == zb[k].dtype and np.array_equal(za[k], zb[k]), (f, k)


@pytest.mark.gpu
def test_cli_gpu_lz_writer_equals_sync_writer(tmp_path, cuda_device):
    a, b = str(tmp_path / "lz"), str(tmp_path / "sync")
    args = ["--n-images", "1", "--height", "24", "--width", "32", "--epochs", "1"]
    r = pp.main(args + ["--out", a, "--writer", "gpu-lz"])
    pp.main(args + ["--out", b, "--writer", "sync"])
    assert r["writer"] == "gpu-lz" and r["files"] == 121
    fa = {os.path.relpath(os.path.join(d, f), a) for d, _, fs in os.walk(a) for f in fs}
    fb = {os.path.relpath(os.path.join(d, f), b) for d, _, fs in os.walk(b) for f in fs}
    assert fa == fb and len(fa) == 121
    for k in sorted(fa):
        za, zb = np.load(os.path.join(a, k)), np.load(os.path.join(b, k))
        assert sorted(za.files) == sorted(zb.files), k
        for m in za.files:
            assert za[m].dtype == zb[m].dtype and np.array_equal(za[m], zb[m]), (k, m)
