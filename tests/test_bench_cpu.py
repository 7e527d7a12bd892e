"""bench.py's host-side helpers (no GPU): the --dump-outputs writer, the options that only --full serves."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('pvr_bench', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_stays_under_64_mb_with_a_fixed_row_sample(tmp_path):
    bench = _bench()
    big = np.random.default_rng(1).standard_normal((9000, 2048)).astype(np.float32)        # 73.7 MB: more than the whole budget
    small = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'big': torch.from_numpy(big), 'small': small})
    total = sum(os.path.getsize(str(tmp_path / 'a' / f)) for f in os.listdir(str(tmp_path / 'a')))
    assert sorted(os.listdir(str(tmp_path / 'a'))) == ['big.npy', 'small.npy'] and total <= 64 * 10 ** 6
    a, b = np.load(str(tmp_path / 'a' / 'big.npy')), np.load(str(tmp_path / 'b' / 'big.npy'))
    assert a.dtype == np.float32 and a.shape[1] == 2048 and 1000 < a.shape[0] < 9000
    assert np.array_equal(a, b)                                                             # the same sample on every run
    rows = {r.tobytes(): i for i, r in enumerate(big)}
    idx = [rows[r.tobytes()] for r in a]                                                    # whole rows of the output, in row order
    assert idx == sorted(idx) and len(set(idx)) == len(idx)
    s = np.load(str(tmp_path / 'a' / 'small.npy'))
    assert s.dtype == np.float64 and np.array_equal(s, small.numpy())                      # small outputs are written whole


def test_roofline_options_are_refused_without_full():
    """--per-op and --dump-plan come from the roofline passes, which only --full runs: a plain run refuses them before it touches a GPU
    instead of ignoring them."""
    for extra in (['--per-op'], ['--dump-plan', 'plan.json']):
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '4'] + extra, capture_output=True, text=True, timeout=300,
                             cwd=ROOT)
        assert out.returncode == 2 and '--full' in out.stderr, out.stderr[-2000:]
