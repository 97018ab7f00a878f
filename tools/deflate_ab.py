"""A/B of the GPU deflate's two modes on real product planes: compressed size
per plane kind, and call time.

The planes come from PreprocessPlusAugment.run_batch on synth inputs at the
product shape (a capturing writer keeps the group tensor [44,H,W] and, of
group 0, one pair of [8,H,W] augment arrays per augmentation kind).  Sizes:
the literal encoder (ofd_deflate_batch), the match mode (ofd_deflate_lz_batch)
for every candidate-distance set ({E}, {1,E}, {E,2E}, {1,E,2E}), host zlib
level 1 and level 6, all on the same bytes.  Times: device events around one
call on B arrays of [8,H,W] f64 and on the [44,H,W] group, warmed, the modes
alternated in one process, several rounds, median and spread.

usage: python tools/deflate_ab.py [B H W] [--rounds R] [--no-zlib]
"""
import argparse
import statistics
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from opticalflowfromdepth_amd import _native, preprocess as pp, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("shape", nargs="*", type=int, default=[2, 768, 1024])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--no-zlib", action="store_true")
args = ap.parse_args()
B, H, W = (args.shape + [2, 768, 1024][len(args.shape):])[:3]
dev = torch.device("cuda:0")
lib = _native.lib()
print(f"build id {_native.build_id()}  B={B} {H}x{W}  rounds={args.rounds}", flush=True)

CANDS = {0: "{E}", 1: "{1,E}", 2: "{E,2E}", 3: "{1,E,2E}"}
GROUP_NAMES = [n for img in ("img0", "img1", "img2", "img3", "img2p", "img3p") for n in (img,) * 3 + (img + "_depth",)] + \
              [n for f in ("flow01", "back_flow01", "flow12", "back_flow12", "flow02", "back_flow02p", "flow03",
                           "back_flow03", "flow13", "back_flow13p") for n in (f,) * 2]


class Capture:
    """The writer interface run_batch needs; keeps device copies instead of writing."""

    def __init__(self):
        self.group, self.aug = None, {}

    def save_batch(self, paths, x, key="img_depth_flow", extra=None):
        name = paths[0].rsplit("/", 1)[1]
        if name == "group.npz":
            self.group = x.clone()
        elif name.startswith("0_"):
            kind = int(extra["augment_flow_type"])
            self.aug.setdefault((kind, name[-5]), x.clone())

    def flush(self):
        pass


class Deflater:
    def __init__(self):
        self.buf = {}

    def _tensors(self, count, bound, each):
        # one set of buffers for both modes, so a timed call never allocates
        k = (count, bound)
        nws = max(lib.ofd_deflate_workspace_bytes(count, each), lib.ofd_deflate_lz_workspace_bytes(count, each))
        if k not in self.buf:
            self.buf = {k: (torch.empty(count * bound, dtype=torch.uint8, device=dev),
                            torch.empty(count, dtype=torch.int64, device=dev),
                            torch.empty(count, dtype=torch.int32, device=dev),
                            torch.empty(max(nws, 256), dtype=torch.uint8, device=dev))}
        return self.buf[k]

    def call(self, x, lz):
        """One call on x [count, ...]; returns the device sizes tensor (no sync)."""
        count, each = x.shape[0], int(x[0].numel() * x.element_size())
        bound = max(lib.ofd_deflate_lz_bound(each), lib.ofd_deflate_bound(each))
        nws = (lib.ofd_deflate_lz_workspace_bytes if lz else lib.ofd_deflate_workspace_bytes)(count, each)
        out, sizes, crcs, ws = self._tensors(count, bound, each)
        tail = (out.data_ptr(), sizes.data_ptr(), crcs.data_ptr(), ws.data_ptr(), nws,
                torch.cuda.current_stream().cuda_stream)
        if lz:
            rc = lib.ofd_deflate_lz_batch(x.data_ptr(), count, each, x.element_size(), *tail)
        else:
            rc = lib.ofd_deflate_batch(x.data_ptr(), count, each, *tail)
        _native.check(rc, "deflate")
        return sizes

    def sizes(self, x, lz):
        s = self.call(x, lz)
        torch.cuda.synchronize()
        return s.cpu().tolist()

    def time_ms(self, x, lz):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.call(x, lz)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)


def kind_of(name, plane):
    if name.endswith("_depth"):
        return "depth"
    if name.startswith("img"):
        return "image"
    if name in ("flow01", "back_flow01"):
        return "disparity flow"
    return "masked flow"


def classify(plane):
    """A plane of an augment array, by content."""
    u = torch.unique(plane[::7, ::5])
    if u.numel() <= 2 and bool(((u == 0) | (u == 1)).all()):
        return "mask"
    if bool((plane == plane.round()).all()) and float(plane.min()) >= 0 and float(plane.max()) <= 255:
        return "image"
    return "depth / flow"


# ---------------------------------------------------------------- the planes
seeds = [12345 + i for i in range(B)]
img0 = synth.synthetic_rgb(seeds, H, W, dev)
depth = synth.synthetic_depth(seeds, H, W, dev, dtype=torch.float64)
cap = Capture()
ppa = pp.PreprocessPlusAugment(dev)
# run_batch's own steps, with the augmentations of group 0 only
params = [pp.draw_image_params(int(s), H, W, pp.AUGMENT_SCHEDULE) for s in seeds]
group44, groups = ppa.stage_one(img0, depth, params)
cap.save_batch(["x/group.npz"], group44)
for g, a, kind, d1, d2 in ppa.augment(groups[:1], params):
    for k, x in (("1", d1), ("2", d2)):
        cap.save_batch([f"x/{g}_{a}_{k}.npz"], x, extra={"augment_flow_type": np.array(kind)})
torch.cuda.synchronize()
del groups, group44

dfl = Deflater()
rows = {}  # kind -> [raw, literal, lz0..lz3, zlib1, zlib6]


def add(kind, planes):
    """planes [count, H, W]: every plane deflated as one array."""
    raw = planes[0].numel() * planes.element_size() * planes.shape[0]
    r = rows.setdefault(kind, [0] * 8)
    r[0] += raw
    r[1] += sum(dfl.sizes(planes, False))
    for m in CANDS:
        lib.ofd_deflate_lz_set_candidates(m)
        r[2 + m] += sum(dfl.sizes(planes, True))
    lib.ofd_deflate_lz_set_candidates(3)
    if not args.no_zlib:
        for p in planes.cpu().numpy():
            b = p.tobytes()
            r[6] += len(zlib.compress(b, 1))
            r[7] += len(zlib.compress(b, 6))


def report(title):
    print(f"\n{title}\n{'kind':<22}{'MB':>8}{'literal':>9}" + "".join(f"{'lz' + c:>11}" for c in CANDS.values())
          + f"{'zlib1':>8}{'zlib6':>8}   (ratios: raw / compressed)")
    tot = [0] * 8
    for kind, r in list(rows.items()) + [("all", None)]:
        if r is None:
            r = tot
        else:
            tot = [a + b for a, b in zip(tot, r)]
        print(f"{kind:<22}{r[0] / 1e6:>8.1f}" + "".join(f"{(r[0] / v if v else float('nan')):>{wd}.2f}"
                                                          for v, wd in zip(r[1:], (9, 11, 11, 11, 11, 8, 8))), flush=True)
    rows.clear()


g0 = cap.group[0]  # [44, H, W] of image 0
for i in range(44):
    add(kind_of(GROUP_NAMES[i], g0[i]), g0[i:i + 1])
report(f"group.npz planes of image 0 ([44,{H},{W}] {str(g0.dtype).replace('torch.', '')}), each plane one stream")
for (kind, k), x in sorted(cap.aug.items()):
    for i in range(8):
        add(f"aug{kind} file{k} {classify(x[0, i])}", x[0, i:i + 1])
report("augment arrays of image 0, group 0 ([8,H,W] each), one pair per augmentation kind, planes by content")

# whole arrays, as the writer deflates them
lz_total = {}
for label, x in [("group [44,H,W] x B", cap.group)] + [(f"aug{kind} file{k} [8,H,W] x B", x)
                                                         for (kind, k), x in sorted(cap.aug.items())]:
    raw = x.numel() * x.element_size()
    lit = sum(dfl.sizes(x, False))
    lz = sum(dfl.sizes(x, True))
    lz_total[label] = (raw, lit, lz)
print("\nwhole arrays as the writer sends them (default candidates {1,E,2E})")
for label, (raw, lit, lz) in lz_total.items():
    print(f"{label:<28} raw {raw / 1e6:8.1f} MB  literal {raw / lit:5.2f}x  lz {raw / lz:5.2f}x  "
          f"lz / literal bytes {lz / lit:5.3f}")

# ---------------------------------------------------------------- call times
print(f"\ncall time, device events, warmed, modes alternated, {args.rounds} rounds: median [min .. max] ms")
some = sorted(cap.aug.items())[0][1]
x8 = some if some.shape[0] >= 8 else some.repeat((8 + some.shape[0] - 1) // some.shape[0], 1, 1, 1)[:8].contiguous()
for label, x in ((f"8 arrays [8,{H},{W}] f64 ({x8.numel() * 8 / 1e6:.0f} MB)", x8),
                 (f"{cap.group.shape[0]} arrays [44,{H},{W}] ({cap.group.numel() * cap.group.element_size() / 1e6:.0f} MB)",
                  cap.group)):
    modes = [("literal", False, 3)] + [("lz" + CANDS[m], True, m) for m in (3, 1, 0, 2)]
    t = {n: [] for n, _, _ in modes}
    for r in range(args.rounds + 1):
        for n, lz, m in modes:
            lib.ofd_deflate_lz_set_candidates(m)
            ms = dfl.time_ms(x, lz)
            if r:  # round 0 warms
                t[n].append(ms)
    lib.ofd_deflate_lz_set_candidates(3)
    print(label)
    gb = x.numel() * x.element_size() / 1e9
    for n, v in t.items():
        med = statistics.median(v)
        print(f"  {n:<14}{med:8.3f} [{min(v):.3f} .. {max(v):.3f}]  {gb / med * 1e3:7.1f} GB/s in")
