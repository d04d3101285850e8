"""The host side of the shared planar stage (woft_amd/planar.py) and the config-key helpers, without a GPU: the result block's
layout, the pure decoder's rules on hand-filled blocks, the bounded buffer cache, config_get / config_set."""
import numpy as np
import pytest
import torch

from woft_amd import ops
from woft_amd.config import Config, config_get, config_set
from woft_amd.planar import BoundedCache, ResultBlock, _Fit, block_views, block_words, decode

MIN_FRAC = 0.2
SPEC = dict(min_frac=MIN_FRAC)


def _filled(K, with_hist, status, frac, seed=0):
    """-> (the block as numpy float32, its named views) with H[t] = t * 10 + 0..8, count rows 100 + t / 200 + t, hist[t] = t + arange."""
    blk = np.zeros(block_words(K, with_hist), np.float32)
    v = block_views(blk, blk.view(np.int32), K, with_hist)
    for t in range(K):
        v.H[t] = 10 * t + np.arange(9)
        v.frac[t], v.status[t] = frac[t], status[t]
        v.selected[t], v.kept[t] = 100 + t, 200 + t
        if with_hist:
            v.hist[t] = t + np.arange(ops.CHAIN_HIST)
    return blk, v


def test_decoder_on_a_three_target_block_with_histograms():
    above = np.nextafter(np.float32(MIN_FRAC), np.float32(1))
    blk, v = _filled(3, True, status=[0, 1, 2], frac=[np.float32(MIN_FRAC), 0.9, above])
    v.H[2] = np.nan                                                  # (status 2: no model, H all NaN)
    out = decode(blk, 3, SPEC, True)
    assert len(out) == 3
    (f0, s0, k0, h0), (f1, s1, k1, h1), (f2, s2, k2, h2) = out
    assert isinstance(f0, _Fit) and f1 is None and isinstance(f2, _Fit)          # status 0, 1, 2
    assert f0.success is False                                       # frac == min_frac in fp32: not above
    assert f2.success is True and np.all(np.isnan(f2.H))             # the next fp32 value above; the NaN H comes through
    assert (s0, s1, s2) == (100, 101, 102) and (k0, k1, k2) == (200, 201, 202)   # the two count rows
    for t, h in enumerate((h0, h1, h2)):
        assert h.dtype == np.int64 and np.array_equal(h, t + np.arange(ops.CHAIN_HIST))
    assert f0.H.dtype == np.float64 and f0.H.shape == (3, 3) and np.array_equal(f0.H, np.arange(9.0).reshape(3, 3))
    assert not np.shares_memory(f0.H, blk)                           # a copy, not a view of the mirror
    blk[:9] = -1.0
    assert np.array_equal(f0.H, np.arange(9.0).reshape(3, 3))


def test_decoder_on_a_single_target_block_without_histogram():
    assert block_words(1, False) == 13
    for frac, want in ((np.float32(MIN_FRAC), False), (np.nextafter(np.float32(MIN_FRAC), np.float32(1)), True)):
        blk, _ = _filled(1, False, status=[0], frac=[frac])
        (fit, selected, kept, hist), = decode(blk, 1, SPEC, False)
        assert fit.success is want and (selected, kept) == (100, 200) and hist is None
        assert np.array_equal(fit.H, np.arange(9.0).reshape(3, 3)) and fit.H.dtype == np.float64
    blk, _ = _filled(1, False, status=[1], frac=[0.9])
    assert decode(blk, 1, SPEC, False) == [(None, 100, 200, None)]


@pytest.mark.parametrize("const", [True, False])
def test_constant_verdict_overrides_the_inlier_fraction(const):
    spec = dict(SPEC, const_verdict=const)
    blk, _ = _filled(3, True, status=[0, 1, 2], frac=[0.0, 1.0, 1.0])
    out = decode(blk, 3, spec, True)
    assert out[0][0].success is const and out[1][0] is None and out[2][0].success is const
    assert decode(blk, 3, dict(const_verdict=const), True)[0][0].success is const        # (min_frac is not read)


@pytest.mark.parametrize("with_hist", [False, True])
@pytest.mark.parametrize("K", [1, 3, 32])
def test_named_views_tile_the_allocation(K, with_hist):
    b = ResultBlock(K, "cpu", with_hist)
    assert b.dev.numel() == block_words(K, with_hist) == K * (13 + (ops.CHAIN_HIST if with_hist else 0))
    assert not b.dev.any() and b.host is None
    base = b.dev.data_ptr()
    parts = [b.H, b.frac, b.status, b.selected, b.kept] + ([b.hist] if with_hist else [])
    assert (b.hist is None) == (not with_hist)
    at = 0
    for p in parts:                                                  # in order, each starting where the last one ended
        assert p.is_contiguous() and p.element_size() == 4 and p.data_ptr() == base + 4 * at
        at += p.numel()
    assert at == b.dev.numel()
    assert tuple(b.H.shape) == (K, 9) and tuple(b.count.shape) == (2, K) and b.count.data_ptr() == b.selected.data_ptr()
    assert b.H.dtype == b.frac.dtype == torch.float32 and b.status.dtype == b.count.dtype == torch.int32
    if with_hist:
        assert tuple(b.hist.shape) == (K, ops.CHAIN_HIST) and b.hist.dtype == torch.int32


def test_bounded_cache():
    made = []

    def make(k):
        def f():
            made.append(k)
            return object()
        return f
    c = BoundedCache(3)
    a = c.lookup("a", make("a"))
    c.lookup("b", make("b"))
    c.lookup("c", make("c"))
    assert c.lookup("a", make("a")) is a and made == ["a", "b", "c"] and len(c) == 3     # a hit makes nothing (and is now the newest)
    c.lookup("d", make("d"))                                            # at the limit: the oldest goes, "b"
    assert "b" not in c and "a" in c and "c" in c and "d" in c and len(c) == 3
    c.lookup("e", make("e"))
    assert "c" not in c and len(c) == 3 and c.get("c") is None and c.get("a") is a
    one = BoundedCache()                                             # limit 1: a new key replaces
    x = one.lookup(1, make(1))
    y = one.lookup(2, make(2))
    assert len(one) == 1 and 1 not in one and one.get(2) is y and list(one.values()) == [y] and x is not y
    one.put(3, x)
    assert len(one) == 1 and one.get(3) is x and one.get(2) is None


class Foreign:
    """Another config class with the reference's semantics: a missing attribute reads as an empty, falsy instance."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return Foreign()

    def __bool__(self):
        return False


@pytest.mark.parametrize("cls", [Config, Foreign])
def test_config_get_and_set(cls):
    C = cls()
    C.none, C.false, C.zero, C.value, C.child = None, False, 0, "gate", cls()
    assert config_get(C, "absent", 7) == 7 and config_get(C, "absent") is None and not config_set(C, "absent")
    assert config_get(C, "none", 7) == 7 and not config_set(C, "none")
    assert config_get(C, "false", 7) is False and not config_set(C, "false")
    assert config_get(C, "zero", 7) == 0 and config_get(C, "zero", 7) is not False and not config_set(C, "zero")
    assert config_get(C, "value", 7) == "gate" and config_set(C, "value") is True
    assert config_get(C, "child", 7) == 7 and not config_set(C, "child")      # (an empty config is what an absent key reads as)
