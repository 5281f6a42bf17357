"""The run-time knobs' one table (csrc/knobs.hip) through mq_tune / mq_tune_get, and tests/knobs.py on top of them.  No GPU: the library loads and
answers these without one.  The rows below are written out here, not read from the library: key, environment variable, built-in default."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from marqo_amd import _lib as L
from tests import knobs

KNOBS = [
    ("gemm_mt", "MQ_GEMM_MT", 0), ("gemm_cgroup", "MQ_GEMM_CGROUP", 8), ("gemm_nh", "MQ_GEMM_NH", 0), ("gemm_tail", "MQ_GEMM_TAIL", 0),
    ("gemm_wd", "MQ_GEMM_WD", 0), ("rs_finalize", "MQ_GEMM_RS_FIN", 0), ("row_select", "MQ_ROW_SELECT", 1), ("ln_fold", "MQ_LN_FOLD", 2),
    ("subln_fold", "MQ_SUBLN_FOLD", 1), ("attn_proj", "MQ_ATTN_PROJ", 128), ("panel_gemm", "MQ_PANEL_GEMM", 0),
    ("residual_bf16", "MQ_RESIDUAL_BF16", 0), ("pool_strided", "MQ_POOL_STRIDED", 1), ("assemble_stats", "MQ_ASSEMBLE_STATS", 1),
    ("small_m", "MQ_SMALL_M", 80), ("small_m_grouped", "MQ_SMALL_M_GROUPED", 320), ("ln_prefetch", "MQ_LN_PREFETCH", 1), ("ln_rows", "MQ_LN_ROWS", 2),
    ("ln_bf16_wide", "MQ_LN_BF16_WIDE", 1), ("xcd_band", "MQ_XCD_BAND", 1), ("attn_waves", None, 0), ("gemm_addr_limit_mb", None, 0),
]
assert len(KNOBS) == 22 and len({k for k, _, _ in KNOBS}) == 22 and sum(e is not None for _, e, _ in KNOBS) == 20

# a fresh interpreter that only loads the library (argv: its path, then the keys) and prints {key: value}
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
out = {}
for key in sys.argv[2:]:
    v = ctypes.c_int(-12345)
    assert lib.mq_tune_get(key.encode(), ctypes.byref(v)) == 0, key
    out[key] = v.value
print(json.dumps(out))
"""


def _fresh_process_values(**env):
    """every key's value in a child process whose environment has no MQ_* variable but those given"""
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("MQ_")}
    child_env.update(env)
    res = subprocess.run([sys.executable, "-c", _CHILD, str(L.LIB_PATH)] + [k for k, _, _ in KNOBS], capture_output=True, text=True, env=child_env,
                         timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout)


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def fresh_defaults():
    return _fresh_process_values()


@pytest.mark.parametrize("key,env,default", KNOBS)
def test_default_set_get_and_restore(lib, fresh_defaults, key, env, default):
    assert fresh_defaults[key] == default
    was = knobs.get(key)
    try:
        for v in (default + 3, default + 7):
            assert lib.mq_tune(key.encode(), v) == L.MQ_OK
            assert knobs.get(key) == v
    finally:
        assert lib.mq_tune(key.encode(), was) == L.MQ_OK
    assert knobs.get(key) == was


def test_gemm_nh_and_the_fp8_big_tile_are_two_variables():
    """mq_tune("gemm_nh", v) also writes the fp8 big-tile switch (v, 4 as 0), which has no key; gemm_nh reads back the bf16 value.  That the two are
    separate variables shows from the outside only through the environment: MQ_GEMM_FP8_NH initialises the one, gemm_nh reads the other."""
    with knobs.tuned(gemm_nh=3):
        assert knobs.get("gemm_nh") == 3
        knobs.tune(gemm_nh=4)
        assert knobs.get("gemm_nh") == 4
    assert _fresh_process_values(MQ_GEMM_FP8_NH="3")["gemm_nh"] == 0


def test_gemm_addr_limit_mb_reads_back_in_mb():
    with knobs.tuned(gemm_addr_limit_mb=2):
        assert knobs.get("gemm_addr_limit_mb") == 2
        knobs.tune(gemm_addr_limit_mb=0)
        assert knobs.get("gemm_addr_limit_mb") == 0


def test_unknown_and_null_keys_are_refused(lib):
    v = C.c_int(7)
    for who, call in ((b"mq_tune", lambda key: lib.mq_tune(key, 1)), (b"mq_tune_get", lambda key: lib.mq_tune_get(key, C.byref(v)))):
        for key in (b"no_such_knob", None):
            assert call(key) == -1
            assert lib.mq_last_error().startswith(who + b": unknown key"), lib.mq_last_error()
    assert lib.mq_tune(b"no_such_knob", 1) == -1 and lib.mq_last_error() == b"mq_tune: unknown key no_such_knob"
    assert lib.mq_tune_get(b"xcd_band", None) == -1 and v.value == 7


def test_every_environment_variable_initialises_its_knob():
    """one child process with all twenty variables set, each to a small non-default value of its own"""
    values = {env: str(3 + i) for i, (_, env, _) in enumerate(e for e in KNOBS if e[1])}    # 3 .. 22: none is 0, 1, 2, 8, 80, 128 or 320
    assert len(values) == 20 and len(set(values.values())) == 20
    assert all(int(values[env]) != default for _, env, default in KNOBS if env)
    got = _fresh_process_values(**values)
    for key, env, _ in KNOBS:
        assert got[key] == (int(values[env]) if env else 0), (key, got[key])


def test_tuned_restores_on_exit_exception_and_half_set():
    was = dict(ln_rows=knobs.get("ln_rows"), xcd_band=knobs.get("xcd_band"))
    knobs.tune(ln_rows=5, xcd_band=6)      # entry values that are neither the defaults nor what the bodies set
    try:
        with knobs.tuned(ln_rows=1, xcd_band=0):
            assert (knobs.get("ln_rows"), knobs.get("xcd_band")) == (1, 0)
        assert (knobs.get("ln_rows"), knobs.get("xcd_band")) == (5, 6)
        with pytest.raises(ZeroDivisionError):
            with knobs.tuned(ln_rows=1, xcd_band=0):
                1 / 0
        assert (knobs.get("ln_rows"), knobs.get("xcd_band")) == (5, 6)
        entered = False
        with pytest.raises(L.MarqoHipError, match="unknown key"):
            with knobs.tuned(ln_rows=1, no_such_knob=1):
                entered = True
        assert not entered and knobs.get("ln_rows") == 5
    finally:
        knobs.tune(**was)
