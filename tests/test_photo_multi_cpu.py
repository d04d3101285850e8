"""The multi-target photometric refinement without a device: every argument the two new entry points reject
is rejected before a launch, the workspace size is the stated one, the new status exists, and PhotoTemplateMulti's option checks
that need no device."""
import ctypes
from pathlib import Path

import numpy as np
import pytest


def _lib():
    from woft_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_workspace_bytes_and_the_new_status():
    from woft_amd import ops
    lib = _lib()
    assert lib.woft_photo_multi_ws_bytes(1, 1) == (68 + 18) * 8 == lib.woft_photo_ws_bytes(40, 40, 1)
    assert lib.woft_photo_multi_ws_bytes(3, 2) == 3 * (2 * 68 + 18) * 8
    assert lib.woft_photo_multi_ws_bytes(32, 5) == 32 * (5 * 68 + 18) * 8
    for K, P in ((0, 1), (1, 0), (-1, 2), (2, -1)):
        assert lib.woft_photo_multi_ws_bytes(K, P) == -1
    assert ops.PHOTO_STATUS_MULTI[5] == "SKIPPED" and ops.PHOTO_STATUS_MULTI[:5] == ops.PHOTO_STATUS
    assert "WOFT_PHOTO_SKIPPED = 5" in (Path(__file__).resolve().parent.parent / "include" / "woft_hip.h").read_text()
    assert ops.photo_multi_partials([(20, 12, 76, 51), (1, 1, 3, 3)], 1) == 2 and ops.photo_multi_partials([(20, 12, 76, 51)], 2) == 1


def test_argument_checks_without_gpu():
    lib = _lib()
    K = 2
    i32s = lambda *v: (ctypes.c_int32 * len(v))(*v)
    f64s = lambda *v: (ctypes.c_double * len(v))(*v)
    eye = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    boxes, W, need, act = i32s(1, 1, 3, 3, 2, 1, 5, 3), f64s(*eye, *eye), i32s(10, 10), i32s(1, 1)
    gains, biases = f64s(1.0, 1.0), f64s(0.0, 0.0)
    p = ctypes.c_void_p(64)                                                  # (never dereferenced: every call is rejected)

    def ev(tmpl=p, bits=p, h=5, w=7, frame=p, hf=9, wf=9, K=K, boxes=boxes, stride=1, W=W, gains=gains, biases=biases, act=act,
           huber=-1.0, ws=p, out=p):
        return lib.woft_photo_eval_multi(tmpl, 0, bits, h, w, None, frame, 0, hf, wf, K, boxes, stride, W, gains, biases, act, 1, huber,
                                         ws, out, None)

    def rf(tmpl=p, bits=p, h=5, w=7, frame=p, hf=9, wf=9, K=K, boxes=boxes, stride=1, W=W, need=need, act=act, iters=3, huber=-1.0,
           eps=1e-3, ws=p, result=p):
        return lib.woft_photo_refine_multi(tmpl, 0, bits, h, w, None, frame, 0, hf, wf, K, boxes, stride, W, need, act, iters, 1, huber,
                                           eps, ws, result, None)

    Wn = f64s(*eye, 1, 0, 0, 0, float("nan"), 0, 0, 0, 1)                    # (the SECOND target's entry)
    Wi = f64s(*eye, 1, 0, float("inf"), 0, 1, 0, 0, 0, 1)
    shared = [dict(tmpl=None), dict(bits=None), dict(frame=None), dict(ws=None), dict(boxes=None), dict(W=None), dict(act=None),
              dict(h=2), dict(w=2), dict(hf=0), dict(wf=0), dict(h=1 << 16, w=1 << 15), dict(hf=1 << 16, wf=1 << 15),
              dict(stride=0), dict(huber=0.0), dict(huber=float("nan")),
              dict(K=0), dict(K=33), dict(K=-1),
              dict(boxes=i32s(1, 1, 3, 3, 2, 1, 7, 3)),                      # the second box leaves the template
              dict(boxes=i32s(1, 1, 3, 3, 2, 1, 5, 5)),
              dict(boxes=i32s(1, 1, 3, 3, -1, 1, 5, 3)),
              dict(boxes=i32s(1, 1, 3, 3, 4, 1, 3, 3)),                      # ... is empty
              dict(boxes=i32s(3, 1, 1, 3, 2, 1, 5, 3)),                      # the first is
              dict(W=Wn), dict(W=Wi)]
    for kw in shared:
        assert ev(**kw) == -1, ("eval", kw)
        assert rf(**kw) == -1, ("refine", kw)
    for kw in (dict(out=None), dict(gains=None), dict(biases=None), dict(gains=f64s(1.0, float("nan"))),
               dict(biases=f64s(float("inf"), 0.0))):
        assert ev(**kw) == -1, kw
    for kw in (dict(result=None), dict(need=None), dict(need=i32s(10, -1)), dict(iters=-1), dict(iters=65), dict(eps=-1.0),
               dict(eps=float("nan")), dict(eps=float("inf"))):
        assert rf(**kw) == -1, kw
    # an inactive target's arguments are still checked; with every target inactive and valid arguments nothing is launched
    off = i32s(0, 0)
    assert rf(act=off, W=Wn) == -1 and ev(act=off, boxes=i32s(1, 1, 3, 3, 2, 1, 7, 3)) == -1
    assert rf(act=off) == 0 and ev(act=off) == 0                             # (p is no address: a launch would have faulted)


def test_python_option_checks():
    import woft_amd
    from woft_amd import photo
    assert woft_amd.PhotoTemplateMulti is photo.PhotoTemplateMulti
    t = np.zeros((8, 9, 3), np.uint8)
    m = np.ones((8, 9), np.uint8)
    bad = [dict(masks=[]), dict(masks=[m] * 33), dict(masks=np.ones((8, 9), np.uint8)), dict(masks=[m], stride=0),
           dict(masks=[m], stride=1.5), dict(masks=[m], stride=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            photo.PhotoTemplateMulti(t, **kw)
