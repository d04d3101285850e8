"""Generate tests/golden/tracker_window_runs.npz by running the REFERENCE's own WOFTWindow (pytracking/tracker/WOFT_window.py of
the reference checkout) on short synthetic sequences.  Run where the reference checkout exists; nothing at test time imports this.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_window_golden.py

Set-up: the stubs of oracle/gen_golden.py (inert cv2 / ipdb, kornia's three functions, 'cuda' -> 'cpu', functional
cv2.warpPerspective / resize / findContours).  WOFT_window.py imports `ltr.data.geom_utils`, a package the reference checkout does
not contain; all it takes from it is `Bbox`, and every method it calls exists under the same name in the reference's own
pytracking/utils/geom_utils.py, which is registered in its place.  THAT THE TWO Bbox CLASSES AGREE IS AN ASSUMPTION.

Recorded per run: per frame H_cur2init, H_global_cur2init, last_good_H2init, H_local_cur2init, lost / N_lost / global_H_success;
the search box and every local box (x, y, w, h).  Frames are not stored (256 x 320 noise textures do not compress): the file
holds the woft_amd.synth arguments and per-frame block sums, and the test regenerates the frames.  The block sums stand in for a
checksum and are compared with a small TOLERANCE, not for equality (tests/test_window_tracker_gpu.py, BLOCK_TOL: 16 grey levels per
32 x 32 x 3 block of ~130 000): synth builds frames with float bicubic interpolation and a final rounding, and another CPU may round
a handful of pixels the other way; a different frame is still caught.

Asserted here: every box, global and local, lies inside the frame as the reference computed it -- the reference slices with a
negative index otherwise, and no golden value may record that.
"""
import os
import sys
import tempfile
from pathlib import Path

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import gen_golden as G  # noqa: E402
from woft_amd import synth  # noqa: E402

BLOCK = 32


def block_sums(img):
    """Per 32 x 32 block (and channel) sum of a (H, W, 3) uint8 image: the frames' checksum in the golden file."""
    h, w, c = img.shape
    a = img[:h // BLOCK * BLOCK, :w // BLOCK * BLOCK].astype(np.int64)
    return a.reshape(h // BLOCK, BLOCK, w // BLOCK, BLOCK, c).sum(axis=(1, 3))


def rect_mask(H, W, r0, r1, c0, c1):
    m = np.zeros((H, W), np.uint8)
    m[r0:r1, c0:c1] = 255
    return m


@torch.no_grad()
def main():
    G.install_stubs()
    G.install_functional_cv2()
    import importlib
    import types
    ref_gu = importlib.import_module("pytracking.utils.geom_utils")            # (the reference's: its checkout leads sys.path)
    assert Path(ref_gu.__file__).is_relative_to(G.REF)
    ltr, ltr_data = types.ModuleType("ltr"), types.ModuleType("ltr.data")
    ltr.data, ltr_data.geom_utils = ltr_data, ref_gu
    sys.modules.update({"ltr": ltr, "ltr.data": ltr_data, "ltr.data.geom_utils": ref_gu})
    from pytracking.tracker.WOFT_window import WOFTWindow
    from pytracking.utils.config import load_config

    grown = []                                     # every box the reference settles on: init's, then one per lost frame
    orig_min = ref_gu.Bbox.with_margins_min_size

    def recording(self, *a, **k):
        b = orig_min(self, *a, **k)
        grown.append([float(b.tl_x), float(b.tl_y), float(b.w), float(b.h)])
        return b
    ref_gu.Bbox.with_margins_min_size = recording

    sd = synth.make_state_dict(seed=7, small=False, weighted=True)
    iters = 4
    out = {"iters": iters, "seed": 7, "block": BLOCK}
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "sd.pth")
        torch.save(sd, model)

        def run(name, H, W, seq_id, frame_ts, mask_rect=None, margin=0.25, force_fail=(), downscale=0):
            conf = load_config(G.REF / "pytracking/configs" / "WOFT.py")
            conf.flow_config.model = model
            conf.flow_config.iters = iters
            conf.flow_config.padding_mode = 'RAFT'        # (a window's size is no multiple of 8: 'nopad' refuses it, raft.py:221-226)
            conf.tracker_class = WOFTWindow
            conf.search_window_margin = margin
            if downscale:
                conf.downscale_inputs = downscale
            state = {"i": 0}
            orig = conf.redet_success_fn

            def redet(*a):
                ok = orig(*a)
                return ok if state["i"] not in force_fail else (ok & False)
            conf.redet_success_fn = redet
            trk = conf.tracker_class(conf)
            template = synth.make_template(H, W, seq_id=seq_id)
            mask = synth.make_init_mask(H, W) if mask_rect is None else rect_mask(H, W, *mask_rect)
            del grown[:]
            trk.init(template, mask)
            k = downscale or 1
            fh, fw = int(round(H / k)), int(round(W / k))                     # the size the tracker works at
            sb = trk.search_bbox
            boxes = [[float(sb.tl_x), float(sb.tl_y), float(sb.w), float(sb.h)]]
            assert len(grown) == (1 if margin else 0)
            Hs, meta, sums, local_boxes = [], [], [block_sums(template)], []
            for i, t in enumerate(frame_ts):
                state["i"] = i
                f = synth.make_frame(template, t)
                sums.append(block_sums(f))
                n0 = len(grown)
                Hc, m = trk.track(f)
                Hs.append(np.asarray(Hc, np.float64))
                loc = getattr(m, "H_local_cur2init", None)
                meta.append([float(bool(m.lost)), float(m.N_lost), float(bool(m.global_H_success)), 0.0 if loc is None else 1.0])
                out[f"{name}_Hglobal_{i}"] = np.asarray(m.H_global_cur2init, np.float64)
                out[f"{name}_lastgood_{i}"] = np.asarray(m.last_good_H2init, np.float64)
                if loc is not None:
                    out[f"{name}_Hlocal_{i}"] = np.asarray(loc, np.float64)
                    lb = grown[n0] if margin else [0.0, 0.0, float(fw), float(fh)]
                    assert len(grown) - n0 == (1 if margin else 0)
                    local_boxes.append([float(i)] + lb)
                    boxes.append(lb)
            # the condition of the golden file: no box leaves the frame, so no value depends on a negative slice index
            for x, y, w, h in boxes:
                assert x >= 0 and y >= 0 and x + w - 1 <= fw - 1 and y + h - 1 <= fh - 1, (name, (x, y, w, h), (fw, fh))
                assert all(float(v).is_integer() for v in (x, y, w, h)), (name, (x, y, w, h))
            if margin:
                assert boxes[0][2] - 1 < fw or boxes[0][3] - 1 < fh, (name, "the window is the whole frame")
            out[f"{name}_synth"] = np.asarray([H, W, seq_id], np.int64)
            out[f"{name}_ts"] = np.asarray(frame_ts, np.int64)
            out[f"{name}_mask"] = mask
            out[f"{name}_margin"] = np.float64(margin or 0.0)
            out[f"{name}_downscale"] = np.int64(downscale)
            out[f"{name}_sums"] = np.stack(sums)
            out[f"{name}_search_box"] = np.asarray(boxes[0], np.float64)
            out[f"{name}_local_boxes"] = np.asarray(local_boxes, np.float64).reshape(-1, 5)
            out[f"{name}_H"], out[f"{name}_meta"] = np.stack(Hs), np.asarray(meta)
            out[f"{name}_force_fail"] = np.asarray(sorted(force_fail), np.int64)
            print(name, "search box", boxes[0], "local", local_boxes, "meta", meta, flush=True)

        run("win", 256, 320, 3, [1, 2, 3, 4, 5])
        run("lost", 256, 320, 4, [1, 2, 3, 4, 5, 6], force_fail=(2, 3))
        run("small", 256, 320, 5, [1, 2, 3], mask_rect=(96, 160, 120, 200), force_fail=(1,))
        run("whole", 256, 320, 6, [1, 2, 3], margin=None, force_fail=(1,))
        run("down", 512, 640, 8, [1, 2, 3], downscale=2, force_fail=(1,))
    out["runs"] = np.asarray(["win", "lost", "small", "whole", "down"])
    path = G.GOLD / "tracker_window_runs.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
