"""Text regions of a page from its label map or colour mask (reference: lib/pc_segmentation.py:get_text_contours, rendered by
lib/render.py:render_morphological): the morphology, the hole filling and the region table run on the device in one call
(pseg_amd.text_regions, include/pseg.h pseg_text_regions); the polygons are crack polygons traced on the host from each region's seed.
Parity with cv2 itself is unpinned (OpenCV is not part of this package's environment); cv2's reversed contour order, the white
islands RETR_CCOMP would also list and cv2's vertex sets are not reproduced.  Image regions (the reference cuts them by XY-cut) and
PAGE-XML are not part of this module."""
import numpy as np

from .colors import ColorMap


class TextRegion:
    """One text region: box (x0, y0, x1, y1), exclusive; area in pixels; seed (y, x), its first pixel in raster order; the crack
    polygon of its outer boundary, (v,2) int32 pixel corners (x, y), clockwise from the seed's top-left corner."""

    def __init__(self, polygon, box, area, seed):
        self.polygon = np.asarray(polygon, np.int32).reshape(-1, 2)
        self.box = tuple(int(v) for v in box)
        self.area = int(area)
        self.seed = tuple(int(v) for v in seed)

    def polygon_coords(self):
        """[(x, y), ...] as PAGE-XML's Coords want them."""
        return [(int(x), int(y)) for x, y in self.polygon]

    def scale(self, factor):
        """This region on a page `factor` times as large: corners scale exactly for an integer factor and are rounded otherwise
        (the area becomes the scaled polygon's)."""
        poly = np.rint(self.polygon.astype(np.float64) * factor).astype(np.int32)
        x, y = poly[:, 0].astype(np.int64), poly[:, 1].astype(np.int64)
        area = int(abs(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)) // 2)
        box = (int(x.min()), int(y.min()), int(x.max()), int(y.max()))
        return TextRegion(poly, box, area, (int(round(self.seed[0] * factor)), int(round(self.seed[1] * factor))))

    def __repr__(self):
        return "TextRegion(box=%r, area=%d, vertices=%d)" % (self.box, self.area, len(self.polygon))


def _label_of(color_map_or_label, name="text"):
    if isinstance(color_map_or_label, ColorMap):
        for rgb, (lid, lname) in color_map_or_label.mapping.items():
            if lname == name:
                return lid
        raise Exception(f"the colour map has no label named {name!r}")
    return int(color_map_or_label)


def regions_of_record(record):
    """The TextRegion list of one pseg_amd.text_regions record: from its "polygons" when it has them (polygons=True: no mask is
    needed), else traced on the host from its mask (masks=True)."""
    from pseg_amd import engine
    polys = record.get("polygons")
    if polys is None:
        polys = engine.trace_regions(record["mask"], record)
    return [TextRegion(p, b, a, s) for p, b, a, s in zip(polys, record["boxes"], record["areas"], record["seeds"])]


def get_text_regions(image, char_height, color_map_or_label, device=0):
    """The text regions of one page.  image: an (H,W) label map, or an (H,W,3) colour mask, which needs a ColorMap and becomes label
    ids through ColorMap.to_labels (its table() must fit a uint8 label map).  color_map_or_label: the ColorMap (the label named
    "text" is taken) or the label id itself.  char_height: the page's line height at the image's scale."""
    from pseg_amd import engine
    img = np.asarray(image)
    if img.ndim == 3:
        if not isinstance(color_map_or_label, ColorMap):
            raise Exception("get_text_regions: a colour mask needs a ColorMap")
        color_map_or_label.table()
        img = color_map_or_label.to_labels(img)
    elif img.ndim != 2:
        raise Exception("get_text_regions: an (H,W) label map or an (H,W,3) colour mask is expected, got shape %r" % (img.shape,))
    how = engine.TextRegions(_label_of(color_map_or_label), char_height=char_height)
    return regions_of_record(engine.text_regions([img], how, device=device)[0])


def render_regions_mask(shape, regions, color):
    """The painted region mask, (H,W,3) uint8: white, every region's polygon filled with `color` (what the reference's
    render_morphological produces for text).  A pixel is painted when its centre lies inside the polygon (even-odd)."""
    H, W = int(shape[0]), int(shape[1])
    out = np.full((H, W, 3), 255, np.uint8)
    for reg in regions:
        x0, y0, x1, y1 = reg.box
        x0, y0, x1, y1 = max(0, x0), max(0, y0), min(W, x1), min(H, y1)
        if x1 <= x0 or y1 <= y0:
            continue
        inside = np.zeros((y1 - y0, x1 - x0), bool)
        poly = reg.polygon
        nxt = np.roll(poly, -1, axis=0)
        for (ax, ay), (bx, by) in zip(poly, nxt):
            if ax == bx and ay != by:                                   # a vertical edge toggles what is right of it
                lo, hi = min(ay, by), max(ay, by)
                inside[max(lo - y0, 0):max(hi - y0, 0), max(ax - x0, 0):] ^= True
        out[y0:y1, x0:x1][inside] = np.asarray(color, np.uint8)
    return out
