"""State fingerprint, host side: the numpy restatement reproduces the known answers computed from the definition,
and the library exports the entry point under ABI 49."""
import numpy as np

import fingerprint_ref as R


def test_restatement_reproduces_the_known_answers():
    f, c = R.fingerprint(np.array([0, 1, 2, 3], dtype=np.uint32))
    assert [int(x) for x in c] == [0xd14a0dda164e9215]
    assert f == 0xb2b8f3852e23cea7
    w = ((np.arange(65537, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.uint32)
    f, c = R.fingerprint(w)
    assert [int(x) for x in c] == [0xbd77ee3b23bb79a2, 0x0f49c86dbf34c4e0]
    assert f == 0xb1d74df72eaa0ad7
    assert R.fingerprint(np.zeros(0, dtype=np.uint32))[0] == 0


def test_restatement_reads_bit_patterns_and_positions():
    a = np.array([0.0, 1.0, 2.0, 3.0], dtype=np.float32)
    b = a.copy()
    b[0] = -0.0
    assert R.fingerprint(R.words_of(a))[0] != R.fingerprint(R.words_of(b))[0]
    assert R.fingerprint(R.words_of(a))[0] != R.fingerprint(R.words_of(a[::-1]))[0]


def test_library_exports_the_entry_point_under_abi_49():
    from mapx import native
    assert native.MAPX_ABI_VERSION == 49
    assert native.lib.mapx_abi_version() == 49
    assert hasattr(native.lib, "mapx_fingerprint_words") and "mapx_fingerprint_words" in native.SIGNATURES
