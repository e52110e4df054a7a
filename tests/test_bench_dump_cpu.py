"""bench.py --dump-outputs on CPU: the files dump_outputs writes (names,
dtypes, shapes, the record fields as columns), the fixed seeded sample above
the size limit, and the option checks of the command line."""
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]


def _parts(n, seed):
    import bench
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, bench.lphy.META_DTYPE)
    rec["cfo"] = rng.standard_normal(n).astype(np.float32)
    rec["t_off"] = rng.integers(-5, 5, n)
    rec["sync_word"] = 0x12
    rec["have_sync"] = 1
    return (rng.integers(0, 128, (n, bench.DATA_SYMS), dtype=np.uint16),
            rng.integers(0, 256, (n, bench.PAYLOAD), dtype=np.uint8),
            rec.view(np.uint8).reshape(n, 32)), rec


def test_dump_outputs_files(tmp_path):
    import bench
    (a, ra), (b, rb) = _parts(5, 1), _parts(3, 2)
    info = bench.dump_outputs(str(tmp_path / "out"), [a, b])
    assert info["frames"] == info["of"] == 8
    got = {p.name: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert sorted(got) == ["payloads.npy", "records.npy", "symbols.npy"]
    assert got["symbols.npy"].dtype == np.float32 and got["payloads.npy"].dtype == np.float32
    assert got["records.npy"].dtype == np.float64
    assert np.array_equal(got["symbols.npy"], np.concatenate([a[0], b[0]]))
    assert np.array_equal(got["payloads.npy"], np.concatenate([a[1], b[1]]))
    names = bench.lphy.META_DTYPE.names
    rec = np.concatenate([ra, rb])
    assert got["records.npy"].shape == (8, len(names))
    for k, name in enumerate(names):
        assert np.array_equal(got["records.npy"][:, k], rec[name].astype(np.float64)), name


def test_dump_outputs_sample_is_fixed_and_within_limit(tmp_path, monkeypatch):
    import bench
    part, _ = _parts(200, 3)
    monkeypatch.setattr(bench, "DUMP_BYTES", 50 * 488)  # room for 50 of the 200 frames
    one = bench.dump_outputs(str(tmp_path / "a"), [part])
    two = bench.dump_outputs(str(tmp_path / "b"), [part])
    assert one["frames"] == two["frames"] == 50 and one["of"] == 200
    idx = np.load(tmp_path / "a" / "frames.npy")
    assert np.array_equal(idx, np.load(tmp_path / "b" / "frames.npy"))
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "symbols.npy"), part[0][idx.astype(int)])
    assert sum(np.load(p).nbytes for p in (tmp_path / "a").iterdir()) <= 50 * 488


def test_sweep_and_csv_need_full():
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--sweep", "--csv", "x.csv"],
                       capture_output=True, text=True)
    assert p.returncode == 2 and "--full" in p.stderr, p.stderr
