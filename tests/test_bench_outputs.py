"""bench.py's plain run, --full and --dump-outputs: a plain run times the
headline only (every other phase's record is null) and --dump-outputs writes
what the last timed step returned, whole or as a fixed seeded sample."""
import json
import os

import numpy as np
import pytest
import torch

import bench


def test_full_is_off_by_default_and_steps_are_checked():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    assert bench.parse(["--full", "--dump-outputs", "d"]).full is True
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_whole_when_small(tmp_path):
    g = torch.Generator().manual_seed(1)
    a = torch.rand(2, 3, 5, 7, generator=g)
    b = torch.rand(2, 1, 5, 7, generator=g).double()
    bench.dump_outputs(str(tmp_path / "d"), [("a", a), ("b", b)])
    assert sorted(os.listdir(tmp_path / "d")) == ["a.npy", "b.npy"]
    ga, gb = np.load(tmp_path / "d" / "a.npy"), np.load(tmp_path / "d" / "b.npy")
    assert ga.dtype == np.float32 and gb.dtype == np.float32
    assert np.array_equal(ga, a.numpy()) and np.array_equal(gb, b.float().numpy())


def test_dump_outputs_samples_within_the_budget_and_repeats(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)  # 1000 values for 8 * 1200 + 1200
    g = torch.Generator().manual_seed(2)
    a = torch.rand(8, 6, 10, 20, generator=g)
    b = torch.rand(8, 1, 10, 15, generator=g)
    named = [("output", a), ("valid", b)]
    bench.dump_outputs(str(tmp_path / "one"), named)
    bench.dump_outputs(str(tmp_path / "two"), named)
    total = 0
    for name, t in named:
        one, two = np.load(tmp_path / "one" / f"{name}.npy"), np.load(tmp_path / "two" / f"{name}.npy")
        assert one.dtype == np.float32 and one.ndim == 1 and np.array_equal(one, two)
        assert one.size == 1000 * t.numel() // (a.numel() + b.numel())  # its share of the budget
        assert np.isin(one, t.numpy()).all()
        total += one.nbytes
    assert total <= 4000
    # another build's different value at a sampled position shows in the dump
    pos = np.sort(np.random.default_rng([bench.DUMP_SEED, 0]).integers(0, a.numel(), size=888, dtype=np.int64))
    assert np.array_equal(np.load(tmp_path / "one" / "output.npy"), a.reshape(-1).numpy()[pos])
    a2 = a.clone()
    a2.view(-1)[int(pos[17])] += 1.0
    bench.dump_outputs(str(tmp_path / "three"), [("output", a2), ("valid", b)])
    assert not np.array_equal(np.load(tmp_path / "three" / "output.npy"), np.load(tmp_path / "one" / "output.npy"))


def test_default_budget_is_under_64_mb():
    assert bench.DUMP_BYTES <= 64 * 1000 * 1000


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_the_last_step(cuda_device, tmp_path, capsys):
    from opticalflowfromdepth_amd import shard, synth
    from oracle import oracle
    B, H, W = 4, 96, 128
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B), "--height", str(H),
            "--width", str(W), "--dump-outputs", str(tmp_path / "out")]
    bench.main(argv)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["metric"] == bench.METRIC and rec["unit"] == "Mpix/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f32"
    assert rec["value"] == pytest.approx(B * H * W / (rec["ms_per_step"] / 1e3) / 1e6, rel=1e-2)
    for phase in ("cpu_baseline", "config2", "hole_fill", "fused_disparity", "fused_ego", "bf16_warp"):
        assert rec[phase] is None, phase
    # the dump is the call's result on the bench's own (seeded) inputs: whole arrays at this size
    seeds = [shard.image_seed(i) for i in range(B)]
    obj, flow, depth = synth.stage_one_batch(seeds, H, W, cuda_device, ego_fraction=0.5)
    exp = oracle.fw_flow(obj.cpu().numpy(), flow.cpu().numpy(), depth.cpu().numpy())
    for name, e in zip(("output", "valid", "collision"), exp):
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == e.shape
        assert np.array_equal(got, e), name
