"""The reference's .osim model files that the registry's recipes name, stored
gzipped under tests/golden/ref_data/ with their relative paths.  The
``ref_data`` fixture unpacks them once per session into a temporary directory
laid out like the reference's data directory (what registry.build_model and
osim.load_osim take)."""
import gzip
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_data')


@pytest.fixture(scope='session')
def ref_data(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('ref_data'))
    n = 0
    for d, _, files in os.walk(GOLDEN):
        for f in files:
            if f.endswith('.osim.gz'):
                dst = os.path.join(out, os.path.relpath(d, GOLDEN), f[:-3])
                os.makedirs(os.path.dirname(dst), exist_ok=True)
                with gzip.open(os.path.join(d, f), 'rb') as src, open(dst, 'wb') as fh:
                    fh.write(src.read())
                n += 1
    assert n == 4, f'{n} model files under {GOLDEN}'
    return out
