"""Frame-features records on the host: the new entry points in the header, EXPORTS and the library, their
argument checks (-1 before any device work), the public names, MultiFlowTracker(share_features=True) against a recording fake
provider (nothing is computed), and the chained tracker's config key."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = ("woft_features_pack", "woft_features_unpack")


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_exports_and_library_agree_on_the_new_names(lib):
    from woft_amd import _lib
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name), name
    assert declared == set(_lib.EXPORTS)
    assert len(_lib._SIGS["woft_features_pack"][1]) == 12 and len(_lib._SIGS["woft_features_unpack"][1]) == 15
    assert lib.woft_abi_version() == raw.woft_abi_version() == 400


def _buffers():
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    return buf, (lambda j: base + 4 * 256 * j)                # (1 KiB apart; only refused calls are made: nothing is dereferenced)


def test_pack_rejects_bad_arguments_without_a_device(lib):
    buf, at = _buffers()
    good = dict(f1=at(0), ld_f1=256, net=at(1), ld_net=128, inp=at(2), ld_inp=256, P=3, fdim=256, hdim=128, cdim=128, record=at(3))
    order = list(good)
    call = lambda **kw: lib.woft_features_pack(*[dict(good, **kw)[n] for n in order], None)
    bad = [dict(f1=None), dict(net=None), dict(inp=None), dict(record=None), dict(P=0), dict(P=-1),
           dict(fdim=0), dict(fdim=-4), dict(fdim=254, ld_f1=256), dict(hdim=126), dict(hdim=0), dict(cdim=66), dict(cdim=0),
           dict(ld_f1=252), dict(ld_f1=0), dict(ld_net=124), dict(ld_inp=124), dict(ld_inp=-256),
           dict(ld_f1=258), dict(ld_net=130), dict(ld_inp=130),          # (rows would leave the 16-byte grid)
           dict(P=1 << 40)]
    for kw in bad:
        assert call(**kw) == -1, kw


def test_unpack_rejects_bad_arguments_without_a_device(lib):
    buf, at = _buffers()
    good = dict(record=at(0), P=3, fdim=256, hdim=128, cdim=128, fmap=at(1), ld_fmap=256, fmap_split=at(2), net=at(3), ld_net=128,
                xbuf=at(4), ld_xbuf=256, inp_c=at(5), ld_inp_c=128)
    order = list(good)
    call = lambda **kw: lib.woft_features_unpack(*[dict(good, **kw)[n] for n in order], None)
    target = dict(fmap_split=None, net=None, xbuf=None, inp_c=None, ld_net=0, ld_xbuf=0, ld_inp_c=0)
    bad = [dict(record=None), dict(fmap=None), dict(P=0), dict(P=-7), dict(fdim=0), dict(fdim=250), dict(hdim=98), dict(cdim=2),
           dict(ld_fmap=252), dict(ld_net=124), dict(ld_xbuf=124), dict(ld_inp_c=124), dict(ld_xbuf=258), dict(ld_net=0),
           # the source role needs all of net, xbuf and inp_c
           dict(net=None), dict(xbuf=None), dict(inp_c=None), dict(net=None, xbuf=None), dict(xbuf=None, inp_c=None),
           # the fused split: contiguous rows of whole 32-channel lines, source role only
           dict(ld_fmap=288), dict(fdim=48, ld_fmap=48), dict(target, fmap_split=at(2)),
           dict(target, record=None), dict(target, fmap=None), dict(target, P=0), dict(target, fdim=6), dict(target, ld_fmap=128),
           dict(P=1 << 40)]
    for kw in bad:
        assert call(**kw) == -1, kw


def test_public_names_resolve():
    import woft_amd
    from woft_amd import flow_provider
    assert woft_amd.FrameFeatures is flow_provider.FrameFeatures
    assert callable(flow_provider.RAFTWrapper.encode_frame)
    rec = SimpleNamespace(numel=lambda: 10, element_size=lambda: 4)
    ff = flow_provider.FrameFeatures("prov", rec, (136, 200, 0, 0), (130, 197))
    assert ff.shape == (130, 197, 3) and ff.geometry == (136, 200, 0, 0) and ff.nbytes == 40 and ff.provider == "prov"


# ---- the tracker against a recording fake provider ---------------------------------------------------------------------------------
class _Record:
    def __init__(self, img):
        self.img = img
        self.shape = tuple(img.shape)


class _FakeProvider:
    """Records its calls; a 'flow' is a zero map."""

    def __init__(self):
        self.C = SimpleNamespace()
        self.pinned, self.calls, self.encoded = None, [], []

    def pin_source(self, img):
        self.pinned = img

    def encode_frame(self, img):
        self.encoded.append(img)
        return _Record(img)

    def compute_flow(self, src, dst, mode=None, do_sigmoid=None, borrow=None, **kw):
        import torch
        assert mode == "flow" and do_sigmoid is False and borrow is True
        self.calls.append((src, dst, kw))
        return torch.zeros(2, *src.shape[:2]), None


class _NoEncodeProvider:
    C = SimpleNamespace()

    def pin_source(self, img):
        pass


def _fake_tracker(monkeypatch, **kw):
    import torch
    from woft_amd import multiflow
    monkeypatch.setattr(multiflow.MultiFlowTracker, "DEVICE", "cpu")
    prov = _FakeProvider()
    trk = multiflow.MultiFlowTracker(prov, **kw)
    log = []

    def fold(best, prev, flow, wl, ml, k, vis_thr, unit_cost, first):
        log.append((k, prev is not None))
        h, w = flow.shape[1:]
        return best or (torch.zeros(2, h, w), torch.zeros(h, w), torch.ones(h, w), torch.zeros(h, w, dtype=torch.int32))
    trk._fold = fold
    return trk, prov, log


def _frame(t):
    return np.full((8, 16, 3), t, np.uint8)


def test_sharing_encodes_every_frame_once_and_hands_out_records(monkeypatch):
    trk, prov, log = _fake_tracker(monkeypatch, share_features=True)
    assert trk.share_features and trk.deltas == (None, 1, 2, 4, 8, 16, 32)
    trk.init(_frame(0))
    # the template is pinned for the direct flows, and encoded once for the chained flows that start at frame 0
    assert prov.pinned is trk._template and len(prov.encoded) == 1 and prov.encoded[0] is trk._template
    assert sorted(trk._records) == sorted(trk._ring) == [0]
    for t in range(1, 37):
        del log[:], prov.calls[:], prov.encoded[:]
        out = trk.track(_frame(t))
        assert out.frame_index == t
        assert len(prov.encoded) == 1 and int(prov.encoded[0][0, 0, 0]) == t                  # exactly once, this frame
        sched = trk.schedule(t)
        assert len(prov.calls) == len(sched) == len(log)
        rec_t = trk._records[t]
        assert isinstance(rec_t, _Record) and rec_t.img is trk._ring[t][0]
        for (src, dst, kw), (k, s, chained) in zip(prov.calls, sched):
            assert kw == {} and dst is rec_t                                                   # the frame's record is every target
            if chained:
                assert isinstance(src, _Record) and int(src.img[0, 0, 0]) == s                 # the stored frame's record
            else:
                assert src is prov.pinned                                                      # the direct flow keeps the pin
        # records live exactly as long as their ring entries, whose shape is unchanged
        assert sorted(trk._records) == sorted(trk._ring) == list(range(max(0, t + 1 - 32), t + 1)), t
        assert all(len(e) == 2 and len(e[1]) == 3 for e in trk._ring.values())
        assert all(trk._records[i].img is trk._ring[i][0] for i in trk._ring)
    trk.reset()
    assert trk._records == {} and trk._ring == {}


def test_chained_sources_are_the_stored_records(monkeypatch):
    trk, prov, log = _fake_tracker(monkeypatch, deltas=(2, 1), share_features=True)
    trk.init(_frame(0))
    kept = {0: trk._records[0]}
    for t in (1, 2, 3, 4):
        del prov.calls[:]
        trk.track(_frame(t))
        kept[t] = trk._records[t]
        for (src, dst, kw), (k, s, chained) in zip(prov.calls, trk.schedule(t)):
            assert chained and src is kept[s] and dst is kept[t]
        assert sorted(trk._records) == sorted(trk._ring) == list(range(max(0, t - 1), t + 1))


def test_without_sharing_nothing_is_encoded(monkeypatch):
    trk, prov, log = _fake_tracker(monkeypatch)
    assert trk.share_features is False
    trk.init(_frame(0))
    for t in range(1, 6):
        trk.track(_frame(t))
    assert prov.encoded == [] and trk._records == {}
    assert all(not isinstance(src, _Record) and not isinstance(dst, _Record) for src, dst, _ in prov.calls)


def test_a_frame_nobody_reads_later_is_still_encoded_once(monkeypatch):
    trk, prov, log = _fake_tracker(monkeypatch, deltas=(None,), share_features=True)
    trk.init(_frame(0))
    assert prov.encoded == []                                                                  # (no chained flow: no record of frame 0)
    trk.track(_frame(1))
    assert len(prov.encoded) == 1 and trk._records == {} and trk._ring == {}
    assert prov.calls[0][0] is prov.pinned and isinstance(prov.calls[0][1], _Record)


def test_a_provider_without_encode_frame_is_refused():
    from woft_amd import MultiFlowTracker
    with pytest.raises(NotImplementedError, match="encode_frame") as e:
        MultiFlowTracker(_NoEncodeProvider(), share_features=True)
    assert "_NoEncodeProvider" in str(e.value)
    MultiFlowTracker(_NoEncodeProvider())                                                     # (the default asks nothing new)


# ---- the chained tracker's key ---------------------------------------------------------------------------------------------------------
class _StubProvider(_FakeProvider):
    def __init__(self, cfg):
        super().__init__()
        self.C = cfg


@pytest.fixture
def on_cpu(monkeypatch):
    from woft_amd import multiflow, tracker
    monkeypatch.setattr(tracker.YAOFTrackerSingleControl, "DEVICE", "cpu")
    monkeypatch.setattr(multiflow.MultiFlowTracker, "DEVICE", "cpu")
    monkeypatch.delenv("WOFT_FUSED", raising=False)


def _tracker(name, **keys):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / name)
    conf.flow_config.of_class = _StubProvider
    for k, v in keys.items():
        setattr(conf, k, v)
    return conf, conf.tracker_class(conf)


def test_shipped_configs_and_the_key(on_cpu):
    from woft_amd.chained import WOFTChained
    from pytracking.utils.config import load_config
    conf, trk = _tracker("WOFT_chained_shared.py")
    assert conf.chain_share_features is True and conf.tracker_class is WOFTChained
    assert trk.chain_share_features is True and trk.multi.share_features is True
    assert "chain_share_features on" in trk.solver_decision
    base = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained.py")
    for k in ("chain_deltas", "chain_vis_thr", "chain_unit_cost", "chain_iters", "chain_weights"):
        assert getattr(conf, k) == getattr(base, k), k
    conf, trk = _tracker("WOFT_chained.py")
    assert isinstance(conf.chain_share_features, type(conf))                                   # (absent: reads as an empty Config)
    assert trk.chain_share_features is False and trk.multi.share_features is False
    assert "chain_share_features off" in trk.solver_decision
    conf, trk = _tracker("WOFT_chained.py", chain_share_features=True)
    assert trk.multi.share_features is True
    # init() builds a fresh MultiFlowTracker: the key survives it
    trk.init(np.zeros((16, 24, 3), np.uint8), np.full((16, 24), 255, np.uint8))
    assert trk.multi.share_features is True and sorted(trk.multi._records) == [0]
