#!/usr/bin/env python
"""Fixture of tests/test_oracle_vs_reference.py FROM THE LIVE REFERENCE: the peak lists per shift and the sorted unique
hashes that the reference's own Analyzer (audfprint_analyze.py, imported unchanged) gives on every seeded case of that
test, with the sha256 of each input, and the reference's file-format constants; and what the reference's Matcher returns
on the random hit lists of tests/test_match_votes.py and its peaks2landmarks / landmarks2hashes on the peak lists of
tests/test_pairing_properties.py, and the module surface / file bytes tests/test_dropin_cpu.py holds the drop-in to.
    python tests/golden/make_golden_refcases.py <directory of the reference's sources>
        -> tests/golden/reference_cases.npz, reference_votes.npz, reference_pairing.npz, reference_dropin.npz"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
from oracle import afp_oracle as O  # noqa: E402
import test_oracle_vs_reference as T  # noqa: E402
import test_match_votes as V  # noqa: E402
import test_pairing_properties as P  # noqa: E402
import test_dropin_cpu as D  # noqa: E402


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    import audfprint_analyze as A  # noqa: E402  (the reference, unchanged)
    out, sha = {}, {}

    def run(key, d, prm, targets=False):
        an = A.Analyzer(prm.density)
        an.maxpksperframe, an.maxpairsperpeak, an.f_sd, an.shifts = prm.maxpksperframe, prm.maxpairsperpeak, prm.f_sd, prm.shifts
        if targets:
            an.targetdf, an.mindt, an.targetdt = prm.targetdf, prm.mindt, prm.targetdt
        pls = [an.find_peaks(d[o:], 11025) for o in O.shift_offsets(prm.shifts)]
        for s, p in enumerate(pls):
            out['%s_peaks%d' % (key, s)] = np.array(p, dtype=np.int32).reshape(-1, 2)
        lms = [A.landmarks2hashes(an.peaks2landmarks(p)) for p in pls]
        hs = np.concatenate(lms) if lms else np.zeros((0, 2), np.int32)
        out[key + '_hashes'] = O.unique_sort_hashes(hs) if len(hs) else np.zeros((0, 2), np.int32)
        sha[key] = T.pcm_sha(d)

    for seed in range(6):
        prm, d = T.random_config_case(seed)
        run('rc%d' % seed, d, prm)
    for seed in range(64):
        prm, clips = T.gpu_suite_case(seed)
        for j, d in enumerate(clips):
            run('gs%d_%d' % (seed, j), d, prm, targets=True)
    for i, d in enumerate(T.unusual_clips()):
        run('un%d' % i, d, O.Params())
    const = dict(PRECOMPEXT=A.PRECOMPEXT, PRECOMPPKEXT=A.PRECOMPPKEXT, HASH_MAGIC=A.HASH_MAGIC.decode(),
                 PEAK_MAGIC=A.PEAK_MAGIC.decode())
    np.savez_compressed(os.path.join(HERE, 'reference_cases.npz'), meta=json.dumps(dict(pcm_sha=sha, constants=const), sort_keys=True),
                        **out)
    print('%d arrays, %d inputs' % (len(out), len(sha)))
    votes(ref_dir)
    pairing(A)
    dropin(A)


def dropin(A):
    import tempfile
    x = D.dropin_inputs()
    v, pk = x['v'], x['pk']
    ra = A.Analyzer()
    fresh = {k: [type(val).__name__, val] for k, val in vars(ra).items()}
    scalars = {}
    for n in D.REF_NAMES:
        val = getattr(A, n)
        if isinstance(val, bytes):
            scalars[n] = dict(bytes=val.decode('latin-1'))
        elif isinstance(val, (int, float, str)):
            scalars[n] = val
    out = dict(locmax=A.locmax(v), locmax_indices=A.locmax(v, indices=True),
               spreadpeaks=ra.spreadpeaks(pk, npoints=256, width=30.0),
               spreadpeaks_base=ra.spreadpeaks(pk[:1], width=7.0, base=np.abs(v[:100])))
    for width in (30.0, 4.0):
        out['spreadpeaksinvector_%g' % width] = ra.spreadpeaksinvector(v[:256], width)
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, 'a.afpt')
        A.hashes_save(f, x['hashes'])
        out['afpt_bytes'] = np.frombuffer(open(f, 'rb').read(), np.uint8)
        hl = [[int(a) for a in t] for t in A.hashes_load(f)]
        A.peaks_save(f, x['peaks'])
        out['afpk_bytes'] = np.frombuffer(open(f, 'rb').read(), np.uint8)
        pl = [[int(a) for a in t] for t in A.peaks_load(f)]
    meta = dict(names=[n for n in D.REF_NAMES if hasattr(A, n)], scalars=scalars,
                analyzer_vars=fresh,
                analyzer_public_vars_after={k: [type(val).__name__, val] for k, val in vars(ra).items() if not k.startswith('_Analyzer__')},
                hashes2landmarks=[[int(a) for a in t] for t in A.hashes2landmarks(x['h'])], hashes_load=hl, peaks_load=pl)
    np.savez_compressed(os.path.join(HERE, 'reference_dropin.npz'), meta=json.dumps(meta, sort_keys=True), **out)
    print('drop-in: %d names, %d scalars' % (len(meta['names']), len(scalars)))


def pairing(A):
    out, sha = {}, {}
    for kind, n in sorted(P.PAIRING_CASES.items()):
        for i in range(n):
            pk, kw = P.pairing_case(kind, i)
            an = A.Analyzer()
            an.maxpairsperpeak, an.targetdf, an.mindt, an.targetdt = kw['maxpairsperpeak'], kw['targetdf'], kw['mindt'], kw['targetdt']
            lm = an.peaks2landmarks([(int(c), int(b)) for c, b in pk])
            k = '%s%d_' % (kind, i)
            out[k + 'landmarks'] = np.array(lm, dtype=np.int64).reshape(-1, 4)
            out[k + 'hashes'] = np.asarray(A.landmarks2hashes(lm))
            sha[k] = P.peaks_sha(pk)
    np.savez_compressed(os.path.join(HERE, 'reference_pairing.npz'), meta=json.dumps(dict(peaks_sha=sha), sort_keys=True), **out)
    print('%d pairing arrays' % len(out))


def votes(ref_dir):
    import audfprint_match as RM  # noqa: E402  (the reference, unchanged)
    out, sha = {}, {}
    for seed in range(8):
        hits, hpi, sw = V.random_hits_case(seed)

        class HT(object):
            hashesperid = hpi
        m = RM.Matcher()
        m.window, m.threshcount, m.search_depth, m.max_alignments_per_id = (sw['window'], sw['threshcount'], sw['search_depth'],
                                                                            sw['max_alignments_per_id'])
        k = 'r%d_' % seed
        rid, rraw = m._best_count_ids(hits, HT)
        out[k + 'ids'], out[k + 'raw'] = rid, rraw
        out[k + 'approx'] = m._approx_match_counts(hits, rid, rraw)
        if m.threshcount >= 1:
            for tr in (False, True):
                m.find_time_range = tr
                out[k + 'exact_t%d' % tr] = m._exact_match_counts(hits, rid, rraw)
        sha['%d' % seed] = V.hits_sha(hits, hpi)
    np.savez_compressed(os.path.join(HERE, 'reference_votes.npz'), meta=json.dumps(dict(hits_sha=sha), sort_keys=True), **out)
    print('%d vote arrays' % len(out))


if __name__ == '__main__':
    main(sys.argv[1])
