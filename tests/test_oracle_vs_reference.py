"""CPU: the oracle against the reference's own outputs on seeded cases -- peak lists per shift and sorted unique hashes
that the UNCHANGED reference Analyzer produced (tests/golden/make_golden_refcases.py, stored in
tests/golden/reference_cases.npz).  The inputs are rebuilt here from their seeds and held against the sha256 of the
samples the reference saw, so the stored outputs answer exactly these inputs."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import afp_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_cases.npz')


def pcm_sha(d):
    return hashlib.sha256(np.ascontiguousarray(d, dtype='<f4').tobytes()).hexdigest()[:16]


# ---- the inputs (shared with the generator) ---------------------------------------------------------------------------
def random_config_case(seed):
    rng = np.random.RandomState(1000 + seed)
    prm = O.Params(density=float(rng.choice([10, 20, 70, 150])),
                   maxpksperframe=int(rng.choice([1, 3, 5, 9])),
                   maxpairsperpeak=int(rng.choice([1, 3, 10])),
                   f_sd=float(rng.choice([10.0, 30.0, 50.0])),
                   shifts=int(rng.choice([1, 1, 2, 4])))
    secs = float(rng.uniform(0.5, 6))
    d = O.synth_noise(seed, secs) if seed % 2 else O.synth_tonal(seed, secs)
    return prm, d


def gpu_suite_case(seed):
    """tests/test_gpu_random_configs.py compares the GPU with the ORACLE on 64 drawn (parameters, clips) cases; here the very
    same cases hold the oracle against the reference (targetdf / mindt / targetdt are Analyzer attributes there too,
    audfprint_analyze.py:139-143).  Clips are cut to 70000 samples to keep the CPU suite short (the GPU test runs them whole)."""
    from test_gpu_random_configs import draw
    kw, clips = draw(seed)
    return O.Params(**kw), [d[:70000] for d in clips]


def unusual_clips():
    """The clips of tests/test_gpu_corners.py::test_unusual_sample_values_equal_the_oracle (tiny / huge gain, DC offset,
    float32 denormals, full-scale square wave, a huge spike in quiet noise)."""
    base = O.synth_noise(4242, 6.0)
    n = len(base)
    spike = (base * np.float32(1e-3)).copy()
    spike[n // 2] = 0.9
    den = (base * np.float32(1e-6)).copy()
    den[100:4000] = np.float32(1e-40) * np.sign(base[100:4000])
    sq = np.where((np.arange(n) // 37) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return [base * np.float32(1e-6), base * np.float32(1e4), (base * np.float32(0.3) + np.float32(0.5)).astype(np.float32),
            den, sq, spike]


# ---- the reference's outputs -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ref():
    z = np.load(GOLDEN)
    return dict(z=z, meta=json.loads(str(z['meta'])))


def _check(ref, key, d, prm, shifts=None):
    """the oracle's peak lists (every shift, or the first `shifts`) and hashes equal the stored reference outputs of `key`"""
    z, meta = ref['z'], ref['meta']
    assert meta['pcm_sha'][key] == pcm_sha(d), 'input of %s differs from the one the reference saw' % key
    op, oh = O.extract(d, prm)
    for s in range(len(op) if shifts is None else shifts):
        assert np.array_equal(z['%s_peaks%d' % (key, s)], op[s]), (key, s)
    assert np.array_equal(z[key + '_hashes'], oh), key


@pytest.mark.parametrize('seed', range(6))
def test_random_configs(ref, seed):
    prm, d = random_config_case(seed)
    _check(ref, 'rc%d' % seed, d, prm)


def test_file_format_constants(ref):
    from audfprint_amd import audfprint_analyze as M
    c = ref['meta']['constants']
    assert c == dict(PRECOMPEXT='.afpt', PRECOMPPKEXT='.afpk', HASH_MAGIC='audfprinthashV00', PEAK_MAGIC='audfprintpeakV00')
    assert (M.PRECOMPEXT, M.PRECOMPPKEXT) == (c['PRECOMPEXT'], c['PRECOMPPKEXT'])
    assert (M.HASH_MAGIC, M.PEAK_MAGIC) == (c['HASH_MAGIC'].encode(), c['PEAK_MAGIC'].encode())


@pytest.mark.parametrize('seed', range(64))
def test_the_gpu_suites_random_cases_hold_for_the_oracle_against_the_live_reference(ref, seed):
    prm, clips = gpu_suite_case(seed)
    for j, d in enumerate(clips):
        _check(ref, 'gs%d_%d' % (seed, j), d, prm)


def test_unusual_sample_values_oracle_equals_the_live_reference(ref):
    prm = O.Params()
    for i, d in enumerate(unusual_clips()):
        _check(ref, 'un%d' % i, d, prm, shifts=1)
