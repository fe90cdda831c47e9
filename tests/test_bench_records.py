"""bench.py's evidence provenance: the rocprofv3 records
it quotes (profiles/traffic.json, profiles/valu.json, written by
tools/ingest_evidence.py) carry the build id of the library they profiled,
and bench.py marks a record of another build ``stale`` (its traffic is then
not quoted).  Host logic only."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_profile_records_are_matched_by_build_id(tmp_path, monkeypatch):
    sys.path.insert(0, REPO)
    import bench
    (tmp_path / 'profiles').mkdir()
    rec = {'bytes': 1.0e7, 'build_id': 'aaaa', 'source': 'profiles/rXX'}
    (tmp_path / 'profiles' / 'traffic.json').write_text(json.dumps({'K/fp64/4096': rec}))
    monkeypatch.setattr(bench, 'REPO', str(tmp_path))
    same = bench._profile_record('traffic.json', 'K/fp64/4096', 'aaaa')
    other = bench._profile_record('traffic.json', 'K/fp64/4096', 'bbbb')
    assert same['stale'] is False and same['bytes'] == 1.0e7
    assert other['stale'] is True
    assert bench._profile_record('traffic.json', 'missing', 'aaaa') is None
    assert bench._profile_record('valu.json', 'K/fp64/4096', 'aaaa') is None


def test_dump_outputs_writes_float_arrays_within_the_cap(tmp_path, monkeypatch):
    """--dump-outputs: one .npy per output, float32 kept and everything else
    float64; past the size cap every array keeps the same seeded sample of env
    rows (rows.npy), identical from call to call."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    n = 100
    outs = {'obs': torch.arange(n * 3, dtype=torch.float32).reshape(n, 3), 'reward': torch.arange(n, dtype=torch.float64),
            'done': (torch.arange(n) % 7 == 0).to(torch.uint8)}
    bench.dump_outputs(str(tmp_path / 'a'), outs)
    got = {k: np.load(tmp_path / 'a' / f'{k}.npy') for k in outs}
    assert (got['obs'].dtype, got['reward'].dtype, got['done'].dtype) == (np.float32, np.float64, np.float64)
    for k in outs:
        np.testing.assert_array_equal(got[k], outs[k].numpy())
    assert not (tmp_path / 'a' / 'rows.npy').exists()
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 40 * (3 * 4 + 8 + 8 + 8))     # room for 40 rows and their indices
    for d in ('b', 'c'):
        bench.dump_outputs(str(tmp_path / d), outs, rank=1)
    rows = np.load(tmp_path / 'b' / 'rows_rank1.npy').astype(int)
    assert len(rows) == 40 and len(set(rows)) == 40 and (np.diff(rows) > 0).all()
    for k in outs:
        b = np.load(tmp_path / 'b' / f'{k}_rank1.npy')
        np.testing.assert_array_equal(b, outs[k].numpy()[rows])
        np.testing.assert_array_equal(b, np.load(tmp_path / 'c' / f'{k}_rank1.npy'))
    total = sum(os.path.getsize(tmp_path / 'b' / f) - 128 for f in os.listdir(tmp_path / 'b'))
    assert total <= bench.DUMP_MAX_BYTES


def test_committed_records_name_their_build():
    """every committed record says which build it measured and where its
    evidence lies"""
    for name in ('traffic.json', 'valu.json'):
        db = json.load(open(os.path.join(REPO, 'profiles', name)))
        for key, rec in db.items():
            if rec.get('build_id') is None:      # round-3 records predate the stamping
                assert rec['source'].startswith('profiles/r03'), (name, key)
                continue
            assert len(rec['build_id']) == 16, (name, key)
            assert os.path.isdir(os.path.join(REPO, rec['source'])), (name, key, rec['source'])
