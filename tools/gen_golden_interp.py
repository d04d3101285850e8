"""Generate tests/golden/flow_interp.npz by running the REFERENCE's pytracking/utils/interpolation.py itself (CPU, fp32).

Run only where the reference checkout is present (the tests read the fixture, never the reference):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_interp.py

The fixture holds, per case, `<case>_data` (C, H, W), `<case>_x`, `<case>_y` (N,), `<case>_interp` = the reference's
bilinear_interpolate_torch(data, x, y) (C, N) and -- for the two-channel cases -- `<case>_warp` = the reference's
flow_warp_coords(stack(x, y), data) (2, N).  Cases:
  * hand_5x7: 2 x 5 x 7 with hand-placed points: exact integers, the last row and column, half-pixels, negatives and 1e9;
  * rand_33x65: 2 x 33 x 65 with 4000 points uniform in [-3, 68] x [-3, 36], a quarter of them rounded to integers;
  * row_1x9 (3 x 1 x 9) and col_9x1 (1 x 9 x 1).
Only finite coordinates with |v| <= 1e9 (beyond int64 the reference's float -> integer conversion is unspecified) and data in
the normal fp32 range.  Arrays only.
"""
import importlib.util
import sys
from pathlib import Path

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
OUT = ROOT / "tests" / "golden" / "flow_interp.npz"


def load_reference():
    sys.path.insert(0, str(REF))                    # (interpolation.py imports pytracking.utils.misc of the reference)
    spec = importlib.util.spec_from_file_location("ref_interpolation", REF / "pytracking" / "utils" / "interpolation.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    rs = np.random.RandomState(20240)
    out = {}
    xs = [0, 1, 6, 5, 3, 2.5, 5.5, 6.5, -0.5, -1, -2.25, 3, 0.25, 5.999, 6.0, 1e9, -1e9, 3, 7, 2, 4.75, 1e9, 0, 6]
    ys = [0, 1, 4, 2, 4, 1.5, 3.5, 2.0, 2.0, -1, 1.5, -0.5, 3.75, 3.999, 4.0, 2, 2, 1e9, 3, 5, 4.5, 1e9, 4, 0]
    out["hand_5x7"] = (rs.normal(0, 1, (2, 5, 7)), np.array(xs), np.array(ys))
    x, y = rs.uniform(-3, 68, 4000), rs.uniform(-3, 36, 4000)
    x[::4], y[::4] = np.round(x[::4]), np.round(y[::4])
    out["rand_33x65"] = (rs.normal(0, 2, (2, 33, 65)), x, y)
    out["row_1x9"] = (rs.normal(0, 1, (3, 1, 9)), rs.uniform(-1, 10, 200), rs.uniform(-1.5, 1.5, 200))
    out["col_9x1"] = (rs.normal(0, 1, (1, 9, 1)), rs.uniform(-1.5, 1.5, 200), rs.uniform(-1, 10, 200))
    return {k: tuple(np.ascontiguousarray(a, dtype=np.float32) for a in v) for k, v in out.items()}


def main():
    ref = load_reference()
    arrays = {}
    for name, (data, x, y) in cases().items():
        assert np.isfinite(x).all() and np.isfinite(y).all() and max(np.abs(x).max(), np.abs(y).max()) <= 1e9
        d, tx, ty = torch.from_numpy(data), torch.from_numpy(x), torch.from_numpy(y)
        interp = ref.bilinear_interpolate_torch(d, tx, ty)
        assert interp.dtype == torch.float32
        arrays.update({f"{name}_data": data, f"{name}_x": x, f"{name}_y": y, f"{name}_interp": interp.numpy()})
        if data.shape[0] == 2:
            arrays[f"{name}_warp"] = ref.flow_warp_coords(torch.stack([tx, ty]), d).numpy()
        if name == "rand_33x65":
            inside = (x > 0) & (x < 64) & (y > 0) & (y < 32)
            print(f"{name}: {100.0 * inside.mean():.1f} % of the points strictly inside")
    np.savez_compressed(OUT, **arrays)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
