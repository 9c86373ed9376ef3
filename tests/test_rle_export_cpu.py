"""Host half of the prediction export: l2s_rle_to_string (maskApi.c:203-215) against the reference's own strings
(tests/golden/ref_rle.npz, ref_rle_live.npz), and the host fallback encoder of model/eval_device.py against the oracle."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import data as OD
from data_util import load_rle_fixture, load_rle_live_fixture


def _cases():
    """[(reference string, reference counts)] of both fixtures"""
    cases, _ = load_rle_fixture()
    return [(c['s'], c['counts']) for c in cases] + [(s, cnt) for s, cnt, _ in load_rle_live_fixture()]


def test_rle_to_string_equals_reference_and_round_trips():
    from lang2seg_amd import ops as O
    cases = _cases()
    assert len(cases) > 40
    for s, cnt in cases:
        out = O.rle_to_string(cnt)
        assert out == s, (out, s)
        assert np.array_equal(O.rle_from_string(out), cnt)
    assert O.rle_to_string(np.zeros(0, np.uint32)) == ''


def test_rle_to_string_differences_of_both_signs():
    """counts behind the third are stored as differences to the count two back: large, negative and zero differences, and the 2^31 range"""
    from lang2seg_amd import ops as O
    for cnt in ([0, 1, 2, 3], [5, 1000000, 1, 2, 999999, 1], [0, 2147483647], [7, 7, 7, 7, 7, 7], [1, 2, 3, 4294967295, 3, 1],
                [15, 16, 17, 31, 32, 33, 1, 0, 1024]):
        c = np.asarray(cnt, np.uint32)
        s = O.rle_to_string(c)
        assert s == OD.rle_to_string(c)
        assert np.array_equal(O.rle_from_string(s), c)


def test_rle_to_string_small_buffer_returns_minus_one():
    """through the raw call: the string and its terminator must fit max_chars"""
    from lang2seg_amd import _lib
    lib = _lib.load()
    s, cnt = max(_cases(), key=lambda c: len(c[0]))
    c = np.ascontiguousarray(cnt, dtype=np.uint32)
    for room, want in ((len(s) + 1, len(s)), (len(s) + 9, len(s)), (len(s), -1), (len(s) // 2, -1), (1, -1), (0, -1)):
        buf = C.create_string_buffer(b'#' * (len(s) + 16), len(s) + 16)
        assert lib.l2s_rle_to_string(c.ctypes.data, c.size, buf, room) == want, room
        if want >= 0:
            assert buf.value.decode('ascii') == s
        assert buf.raw[max(room, 0):] == b'#' * (len(s) + 16 - max(room, 0))       # nothing behind max_chars is touched
    assert lib.l2s_rle_to_string(None, 1, C.create_string_buffer(8), 8) == -1


def test_host_fallback_encoder_equals_oracle():
    from lang2seg_amd.model.eval_device import rle_encode_host
    rs = np.random.RandomState(5)
    masks = [np.zeros((1, 1), np.uint8), np.ones((1, 1), np.uint8), np.zeros((37, 41), np.uint8), np.ones((37, 41), np.uint8),
             (np.indices((37, 41)).sum(0) % 2).astype(np.uint8), (rs.uniform(0, 1, (65, 9)) < 0.5).astype(np.uint8)]
    masks += [c['mask'] for c in load_rle_fixture()[0]]
    for m in masks:
        assert np.array_equal(rle_encode_host(m), OD.rle_encode(m)), m.shape
    assert np.array_equal(rle_encode_host(masks[5] * 200), OD.rle_encode(masks[5]))   # nonzero = 1
