"""Box arithmetic of the search-window tracker (woft_amd.tracker.WOFTWindow): what the reference's WOFT_window.py asks of its
`Bbox` (from_mask, with_margins, intersection, with_margins_min_size, crop_image) and `H_undo_crop`, restated from their
semantics.  Pure numpy / Python: importable without a GPU.

A Box is (tl_x, tl_y, w, h) with an INCLUSIVE bottom-right corner br = tl + size - 1.  Cropping an image by a box is
EXCLUSIVE of that corner: rows [tl_y, br_y), columns [tl_x, br_x) -- a box of width w crops w - 1 columns (the reference
slices `img[tl_y:br_y, tl_x:br_x]`).  The tracker reproduces that, so `crop_rect` is the one place the two conventions meet.
"""
from dataclasses import dataclass

import numpy as np

from .homography import compose_H

MIN_WINDOW = 8 * 20          # smallest search window side the reference grows a box to (WOFT_window.py:41)


def _round_int(x):
    return int(np.round(x))


@dataclass(frozen=True)
class Box:
    tl_x: float
    tl_y: float
    w: float
    h: float

    @property
    def br_x(self):
        return self.tl_x + self.w - 1

    @property
    def br_y(self):
        return self.tl_y + self.h - 1

    @classmethod
    def from_xyxy(cls, tl_x, tl_y, br_x, br_y):
        return cls(tl_x, tl_y, br_x - tl_x + 1, br_y - tl_y + 1)

    @classmethod
    def from_extent(cls, rmin, rmax, cmin, cmax, any_set=True):
        """From the {rmin, rmax, cmin, cmax, any} record of ops.mask_bbox; nothing set: the 1 x 1 box at the origin."""
        if not any_set:
            return cls.from_xyxy(0, 0, 0, 0)
        return cls.from_xyxy(int(cmin), int(rmin), int(cmax), int(rmax))

    @classmethod
    def from_mask(cls, mask):
        """Tight box of the set pixels of a 2-D mask; an all-zero mask gives the 1 x 1 box at the origin."""
        m = np.asarray(mask) != 0
        rows, cols = np.flatnonzero(m.any(axis=1)), np.flatnonzero(m.any(axis=0))
        if rows.size == 0:
            return cls.from_extent(0, 0, 0, 0, any_set=False)
        return cls.from_extent(rows[0], rows[-1], cols[0], cols[-1])

    @classmethod
    def frame(cls, width, height):
        return cls(0, 0, width, height)

    def as_xywh(self):
        return (self.tl_x, self.tl_y, self.w, self.h)

    def with_margins(self, fraction):
        """Grown on every side by int(fraction * size): the product is TRUNCATED, per axis."""
        mx, my = int(fraction * self.w), int(fraction * self.h)
        return Box.from_xyxy(self.tl_x - mx, self.tl_y - my, self.br_x + mx, self.br_y + my)

    def with_margins_min_size(self, min_w, min_h=None):
        """Grown (by ONE margin fraction for both axes: the larger of the two needed) until w >= min_w and h >= min_h."""
        min_h = min_w if min_h is None else min_h
        need = max(max(min_w - self.w, 0) / 2 / self.w, max(min_h - self.h, 0) / 2 / self.h)
        return self.with_margins(need) if need > 0 else self

    def intersection(self, other):
        return Box.from_xyxy(max(self.tl_x, other.tl_x), max(self.tl_y, other.tl_y),
                             min(self.br_x, other.br_x), min(self.br_y, other.br_y))

    def rounded(self):
        return Box.from_xyxy(_round_int(self.tl_x), _round_int(self.tl_y), _round_int(self.br_x), _round_int(self.br_y))

    def inside(self, width, height):
        r = self.rounded()
        return r.tl_x >= 0 and r.tl_y >= 0 and r.br_x <= width - 1 and r.br_y <= height - 1

    def crop_rect(self):
        """(y0, x0, rows, cols) of the crop: corners rounded, bottom-right EXCLUSIVE (rows = h - 1, cols = w - 1)."""
        r = self.rounded()
        return r.tl_y, r.tl_x, r.br_y - r.tl_y, r.br_x - r.tl_x

    def crop_image(self, img):
        y0, x0, rows, cols = self.crop_rect()
        return img[y0:y0 + rows, x0:x0 + cols, ...]


def union_box(boxes):
    """The smallest Box that contains every Box of `boxes` (an iterable; None entries contribute nothing); None when nothing
    contributes.  The one window of the multi-target windowed tracker (woft_amd.chained_multi_window) is chain_rect of this."""
    boxes = [b for b in boxes if b is not None]
    if not boxes:
        return None
    return Box.from_xyxy(min(b.tl_x for b in boxes), min(b.tl_y for b in boxes), max(b.br_x for b in boxes), max(b.br_y for b in boxes))


def search_box(mask_box, margin, width, height, min_size=MIN_WINDOW, clip=True):
    """The window around `mask_box` in a width x height frame (WOFT_window.py:37-44, 215-221): margins, cut to the frame,
    grown to the minimum size.  A falsy margin: the whole frame.
    clip (this project's deviation): the minimum-size step can push a box past the frame edge, where the reference then slices
    with a negative index; here the grown box is cut to the frame once more.  clip=False is the reference's box."""
    frame = Box.frame(width, height)
    if not margin:
        return frame
    box = mask_box.with_margins(margin).intersection(frame).with_margins_min_size(min_size)
    return box.intersection(frame) if clip else box


def check_quantum(quantum):
    """A window quantum -> the int; ValueError unless it is a positive multiple of 8 (the flow provider's feature stride)."""
    if isinstance(quantum, bool) or not isinstance(quantum, (int, np.integer)) or quantum <= 0 or quantum % 8:
        raise ValueError(f"chain_rect: quantum must be a positive multiple of 8, got {quantum!r}")
    return int(quantum)


def chain_rect(mask_box, margin, width, height, quantum=64, min_size=MIN_WINDOW):
    """The rectangle (y0, x0, rows, cols) the windowed chained tracker (woft_amd.chained_window) runs a flow on: the crop of
    search_box(mask_box, margin, ...), with each side grown to a multiple of `quantum` around its centre and pushed back inside
    the frame; a side that would reach the frame's takes the whole side.  A falsy margin: the whole frame, (0, 0, height, width)
    -- every row and column, unlike Box.frame(..).crop_rect(), so that the whole-frame case is WOFTChained's.
    Quantised sides repeat from frame to frame while the box follows the object: the flow provider keeps one plan per padded
    size, so the sizes it meets stay few.  quantum: a positive multiple of 8 (the provider's feature stride)."""
    quantum = check_quantum(quantum)
    width, height = int(width), int(height)
    if not margin:
        return 0, 0, height, width
    y0, x0, rows, cols = search_box(mask_box, margin, width, height, min_size).crop_rect()

    def axis(origin, size, side):
        n = -(-int(size) // quantum) * quantum
        if n >= side:
            return 0, side
        return min(max(int(origin) - (n - int(size)) // 2, 0), side - n), n
    (y0, rows), (x0, cols) = axis(y0, rows, height), axis(x0, cols, width)
    return y0, x0, rows, cols


def H_undo_crop(box, H_window):
    """A homography between two crops by `box` -> the same map in frame coordinates: T(+tl) H T(-tl) for column vectors."""
    to_window = np.array([[1, 0, -box.tl_x], [0, 1, -box.tl_y], [0, 0, 1.0]])
    to_frame = np.array([[1, 0, box.tl_x], [0, 1, box.tl_y], [0, 0, 1.0]])
    return compose_H(to_window, H_window, to_frame)
