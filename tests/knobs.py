"""The one way the tests steer the library's run-time knobs (mq_tune / mq_tune_get, csrc/knobs.hip):
    with tuned(ln_rows=1, xcd_band=0): ...      # on the way out every key is back at the value it had on the way in, whatever happened inside
    tune(row_select=0)                          # a plain set, for the few places that need no scope
What comes back is what mq_tune_get read — the value the process runs with (MQ_* in the environment included), not a built-in default."""
import contextlib
import ctypes as C

from marqo_amd import _lib as L


def get(key: str) -> int:
    v = C.c_int()
    L.check(L.load().mq_tune_get(key.encode(), C.byref(v)), "mq_tune_get")
    return v.value


def tune(**kv):
    for k, v in kv.items():
        L.check(L.load().mq_tune(k.encode(), v), "mq_tune")


@contextlib.contextmanager
def tuned(**kv):
    was = {}
    try:
        for k, v in kv.items():
            was[k] = get(k)
            tune(**{k: v})
        yield
    finally:
        tune(**was)
