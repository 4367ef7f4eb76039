"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run -- only the headline fields, K timed steps -- and what
`--dump-outputs DIR` writes: the rows of the last timed step, equal to the oracle's on the same synthetic clips."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / 'dump'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
           '--nclips', '48', '--secs', '5', '--pool', '48', '--dump-outputs', str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['steps'] == 3 and d['warmup'] == 1 and d['n_gpus'] == 1
    assert d['unit'] == 'hashes/s' and d['higher_is_better'] is True and d['dtype'] == 'f64' and d['value'] > 0
    assert d['ms_per_step'] > 0 and abs(d['value'] - d['hashes_per_step'] / (d['ms_per_step'] * 1e-3)) < 0.01 * d['value']
    for k in ('roofline', 'parity', 'cpu_baseline', 'c5', 'c2_single_clip', 'ranks_seen', 'ms_per_step_one_context'):
        assert k not in d, k
    h, off, clips = (np.load(str(out_dir / f)) for f in ('hashes.npy', 'hash_offsets.npy', 'clips.npy'))
    assert h.dtype == off.dtype == clips.dtype == np.float64
    assert np.array_equal(clips, np.arange(48)) and off[-1] == len(h) == d['hashes_per_step']
    spec = importlib.util.spec_from_file_location('afp_bench_under_test', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from oracle import afp_oracle as O
    pool = bench.synth_pool(48, 5 * bench.SR, seed0=0)
    prm = O.Params(density=20.0, maxpairsperpeak=3, shifts=1)
    for i in (0, 17, 47):
        assert np.array_equal(h[int(off[i]):int(off[i + 1])], O.extract(pool[i], prm)[1].astype(np.float64)), i
