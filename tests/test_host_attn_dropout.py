"""ecgb_attn_fwd_dropout / ecgb_attn_bwd_dropout without a GPU: the symbols are declared and exported, and a call that cannot run is refused by
its argument checks -- head_dim other than 64 with ECGB_ERR_UNSUPPORTED, p outside [0, 1) with ECGB_ERR_INVALID -- before anything touches a device
(the operands are addresses inside one host buffer and are never read; this machine may have no device at all).  Also the numpy mask rule of
tests/dropout_ref.py against values worked out by hand from the definition."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dropout_ref import attn_keep, keep_flat, mix32, threshold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    from ecg_byte_amd import _lib
    return _lib.lib()


def _call(lib, which, head_dim, p, seed=11, ld=None):
    buf = (C.c_uint8 * 8192)()
    a = (C.addressof(buf) + 63) & ~63
    B, S, Hq, Hkv = 2, 64, 4, 2
    QKV = (Hq + 2 * Hkv) * head_dim if ld is None else ld
    if which == "fwd":
        rc = lib.ecgb_attn_fwd_dropout(a, QKV, a + 256, QKV, a + 512, QKV, a + 768, a + 1024, Hq * head_dim, a + 1280, B, S, Hq, Hkv, head_dim, 0.125,
                                       p, seed, None)
    else:
        rc = lib.ecgb_attn_bwd_dropout(a, QKV, a + 256, QKV, a + 512, QKV, a + 768, a + 1024, a + 1280, Hq * head_dim, a + 1536, a + 1792,
                                       a + 2048, QKV, a + 2304, QKV, a + 2560, QKV, B, S, Hq, Hkv, head_dim, 0.125, None, 0, p, seed, None)
    return rc, (lib.ecgb_last_error() or b"").decode()


def test_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "ecgbyte_decoder.h")).read()
    for name in ("ecgb_attn_fwd_dropout", "ecgb_attn_bwd_dropout"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " is not declared in include/ecgbyte_decoder.h"
        fn = getattr(lib, name)                                    # AttributeError: not exported
        plain = getattr(lib, name[: -len("_dropout")])
        assert fn.restype is C.c_int
        # the plain entry point's arguments with (float p, uint64 seed) in front of the stream
        assert list(fn.argtypes) == list(plain.argtypes[:-1]) + [C.c_float, C.c_uint64, C.c_void_p], name
    m = re.search(r"int\s+ecgb_attn_fwd_dropout\s*\(([^;]*)\)\s*;", header)
    assert re.search(r"float\s+p\s*,\s*uint64_t\s+seed\s*,\s*void\s*\*\s*stream\s*$", m.group(1).strip())
    m = re.search(r"int\s+ecgb_attn_bwd_dropout\s*\(([^;]*)\)\s*;", header)
    assert re.search(r"float\s+p\s*,\s*uint64_t\s+seed\s*,\s*void\s*\*\s*stream\s*$", m.group(1).strip())


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_refused_before_any_device_call(lib, which):
    name = f"ecgb_attn_{which}_dropout"
    for hd in (128, 256, 32):
        rc, msg = _call(lib, which, hd, 0.25)
        assert rc == UNSUPPORTED and msg.startswith(name + ":") and "head_dim" in msg, (hd, rc, msg)
    for p in (1.0, -0.1, 1.5, float("nan")):
        rc, msg = _call(lib, which, 64, p)
        assert rc == INVALID and msg.startswith(name + ":"), (p, rc, msg)
    rc, msg = _call(lib, which, 128, 1.0)                          # both wrong: still refused
    assert rc in (INVALID, UNSUPPORTED) and msg.startswith(name + ":")
    # the checks of the plain entry points hold here too: a row stride off 8 elements
    rc, msg = _call(lib, which, 64, 0.25, ld=8 * 64 + 4)
    assert rc == UNSUPPORTED and msg.startswith(name + ":"), (rc, msg)


def test_numpy_mask_rule():
    # splitmix64 by hand in Python integers
    def ref(seed, idx):
        M = (1 << 64) - 1
        z = (seed + idx * 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return (z ^ (z >> 31)) >> 32
    for seed, idx in ((0, 0), (17, 1), (1000003 * 5 + 17 + 7919 * 3 + 4, 2 * 4 * 257 * 257 - 1), (2 ** 63 + 5, 2 ** 33 + 7)):
        assert int(mix32(seed, np.array([idx], dtype=np.uint64))[0]) == ref(seed, idx)
    # p is a float32 in the threshold: 0.1f = 0.100000001490116..., 0.2f = 0.20000000298...
    assert int(threshold(0.25)) == 1 << 30 and int(threshold(0.0)) == 0
    assert int(threshold(0.1)) == int(float(np.float32(0.1)) * 2 ** 32) == 429496736 and int(threshold(0.1)) != int(0.1 * 2 ** 32)
    k = attn_keep(0.25, 99, 2, 3, 70)
    assert k.shape == (2, 3, 70, 70) and k.dtype == np.bool_
    assert np.array_equal(k.reshape(-1), keep_flat(0.25, 99, 2 * 3 * 70 * 70))
    assert k[1, 2, 69, 68] == (ref(99, ((1 * 3 + 2) * 70 + 69) * 70 + 68) >= 1 << 30)
    assert abs(1.0 - k.mean() - 0.25) < 0.01
    assert attn_keep(0.0, 99, 1, 1, 8).all()
