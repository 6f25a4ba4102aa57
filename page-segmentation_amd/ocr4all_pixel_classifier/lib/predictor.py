"""Predictor (reference: lib/predictor.py:10-54): page loop, optional rescale to the original
resolution, post-process chain, mask generation."""
import dataclasses
import os
from typing import Generator

import numpy as np

from .dataset import Dataset, SingleData
from .network import Network, tf_backend_allow_growth
from .output import Masks, generate_output_masks, scale_to_original_shape
from .predictor_data import LazyArray, Prediction, PredictSettings


class Predictor:
    def __init__(self, settings: PredictSettings, network: Network = None):
        self.settings = settings
        self.network = network
        if settings.gpu_allow_growth:
            tf_backend_allow_growth()
        if not network:
            self.network = Network("Predict", n_classes=settings.n_classes,
                                   model=os.path.abspath(self.settings.network))
        if settings.output:
            for sub in ("overlay", "color", "inverted"):
                os.makedirs(os.path.join(settings.output, sub), exist_ok=True)

    # -- the chain on the device (pseg_predict_chain) ---------------------------------------------------------------
    def _chain_ops(self):
        """The post-processor list as chain op ids, or None when a foreign callable is in it (then the host chain runs)."""
        from . import postprocess as pp
        known = {pp.vote_connected_component_class: "cc_vote", pp.add_bounding_boxes: "bbox"}
        ops = []
        for processor in (self.settings.post_process or []):
            if processor not in known:
                return None
            ops.append(known[processor])
        return ops

    def _chain_inputs(self, data: SingleData, want_masks, record=True):
        """What the device chain takes for this page: (data', network input, uint8 binarisation or None, out_shape or None, op
        names), or None when this page / these settings need the host chain (a post-processor that is not one of this package's,
        > 256 classes, no binary for the vote).  record=False (the list path, which reads no data'): the record's image is not
        resized to the original resolution -- the masks need the binarisation alone."""
        net = self.network
        ops = self._chain_ops()
        if ops is None or net.n_classes > 256 or getattr(net, "_rgb", False) and np.asarray(data.image).ndim != 2:
            return None
        image = np.asarray(data.image)
        out_shape = None
        page = data
        binary = data.binary
        if self.settings.high_res_output:
            # lib/output.py:63-79: the image and the binarisation of the record are resized as the reference does (they are
            # not on the hot path); the label map's resize is a stage of the device chain (identity when the shapes agree)
            from .util import preserving_resize
            out_shape = tuple(int(v) for v in data.original_shape[:2])
            resized_image = preserving_resize(data.image, data.original_shape) if record else data.image
            if np.asarray(data.binary).shape != tuple(data.original_shape):
                binary = data.orig_binary if data.orig_binary is not None else preserving_resize(data.binary, data.original_shape).astype('bool')
            page = dataclasses.replace(data, binary=binary, image=resized_image)
        need_bin = want_masks or "cc_vote" in ops
        if need_bin and binary is None:
            return None
        from .util import gray_to_rgb
        img = gray_to_rgb(image) if getattr(net, "_rgb", False) else image
        return page, img, np.asarray(binary).astype(np.uint8) if need_bin else None, out_shape, ops

    def _chain(self, data: SingleData, want_masks: bool, png_level=0):
        """predict -> [scale_to_original_shape] -> post-processors -> [masks] without the label map leaving the device
        (lib/predictor.py:32-54).  Returns (data', labels_u8, masks or None), or None when the host chain has to run (_chain_inputs)."""
        got = self._chain_inputs(data, want_masks)
        if got is None:
            return None
        page, img, binary, out_shape, ops = got
        net = self.network
        res = net.model.predict_chain(img, binary=binary, out_shape=out_shape,
                                      post_ops=ops, exact_labels=net.exact == "labels", labels=None if want_masks else "u8",
                                      lut=self.settings.color_map.lut() if want_masks else None, masks=want_masks,  # True or "png"
                                      png_level=png_level)
        return page, res["labels"], res["masks"]

    def _labels(self, data: SingleData):
        logit, prob, pred = self.network.predict_single_data(data)
        if self.settings.high_res_output:
            data, pred = scale_to_original_shape(data, pred)
        for processor in (self.settings.post_process or []):
            pred = processor(pred, data)
        return data, prob, pred

    #: pages per pseg_predict_batch call in predict(): uploads / downloads of neighbouring pages overlap the compute
    BATCH_PAGES = 8

    def _finish(self, data: SingleData, pred):
        """Everything of _labels() after the network: rescale to the original resolution, post-process chain."""
        page = data
        if self.settings.high_res_output:
            data, pred = scale_to_original_shape(data, pred)
        for processor in (self.settings.post_process or []):
            pred = processor(pred, data)
        prob = LazyArray(lambda page=page: self.network.predict_single_data(page)[1])
        return Prediction(pred, prob, data)

    def predict(self, dataset: Dataset) -> Generator[Prediction, None, None]:
        """lib/predictor.py:27-30, a plain page loop in the reference.  With post-processors or high_res_output every
        page takes the device chain (predict_single); a bare label-map stream takes Network.predict_labels (the
        overlapped batch entry, BATCH_PAGES pages at a time).  Probabilities are fetched on first read."""
        pages = list(dataset.data)
        if (self.settings.post_process or self.settings.high_res_output) and self._chain_ops() is not None:
            for data in pages:
                yield self.predict_single(data)
            return
        for i in range(0, len(pages), self.BATCH_PAGES):
            chunk = pages[i:i + self.BATCH_PAGES]
            for data, pred in zip(chunk, self.network.predict_labels([d.image for d in chunk])):
                yield self._finish(data, pred)

    def predict_single(self, data: SingleData) -> Prediction:
        got = self._chain(data, want_masks=False)
        if got is not None:
            page, lab_u8, _ = got
            # labels: the reference's int64 map, widened on first read; probabilities: fetched on first read
            return Prediction(LazyArray(lambda lab_u8=lab_u8: lab_u8.astype(np.int64)),
                              LazyArray(lambda data=data: self.network.predict_single_data(data)[1]), page)
        data, prob, pred = self._labels(data)
        return Prediction(pred, prob, data)

    def predict_masks(self, data: SingleData) -> Masks:
        got = self._chain(data, want_masks=True)
        if got is not None:
            color, overlay, inverted, fg = got[2]
            return Masks(color=color, overlay=overlay, inverted_overlay=inverted, fg_color_mask=fg)
        data, _, pred = self._labels(data)
        return generate_output_masks(data, pred, self.settings.color_map)

    def write_masks(self, data: SingleData, output_dir=None, level=None):
        """predict_masks + output_data (lib/predictor.py:49-54, lib/output.py:20-41) for ".png" targets as ONE device call:
        predict -> [rescale] -> post-processors -> masks -> PNG (pseg_predict_chain_png); only the three PNG streams come
        down, and they are written to color/, overlay/ and inverted/ under output_dir (default: settings.output) with
        output_data's names.  Other extensions, output.DEVICE_PNG = False and pages that need the host chain go through
        predict_masks' stages and output_data.  level: the device encoder's (0: fixed Huffman codes, 1: a dynamic code per
        band, smaller files); None: output.DEVICE_PNG_LEVEL.  Returns the three paths."""
        from . import output
        level = output.DEVICE_PNG_LEVEL if level is None else level
        output_dir = output_dir if output_dir is not None else self.settings.output
        if output_dir is None:
            raise Exception("write_masks needs an output directory")
        for sub in ("color", "overlay", "inverted"):
            os.makedirs(os.path.join(output_dir, sub), exist_ok=True)
        paths = output.output_paths(output_dir, data)
        if not (output.DEVICE_PNG and output.is_png_target(paths[0])):
            from PIL import Image
            m = self.predict_masks(data)
            for path, mask in zip(paths, (m.color, m.overlay, m.inverted_overlay)):
                Image.fromarray(np.asarray(mask)).save(path)
            return paths
        got = self._chain(data, want_masks="png", png_level=level)
        if got is not None:
            output.write_png_streams(paths, got[2][:3])
            return paths
        data, _, pred = self._labels(data)
        output.output_data(output_dir, np.asarray(pred), data, self.settings.color_map, level=level)
        return paths

    def _list_takes(self, shape):
        """Whether the page-list entries take a page of this shape: they run whole pages only, so a page the whole-page path would
        refuse (Engine.page_fits) goes through write_masks, which tiles it.  A model object without page_fits refuses none."""
        fits = getattr(self.network.model, "page_fits", None)
        return True if fits is None else fits(int(shape[0]), int(shape[1]))

    #: what write_masks_dataset(mixed=None) does with a chunk whose pages differ in shape: True = units by canvas
    #: (Engine.predict_chain_pages(mixed=True)); see DESIGN.md 5c for the measurement this default rests on
    MIXED_DEFAULT = True

    def write_masks_dataset(self, dataset: Dataset, output_dir=None, level=None, chunk_pages=64, mixed=None):
        """write_masks for every page of a dataset (lib/predictor.py:27-30 over :49-54), the pages streamed through the device chain
        chunk_pages at a time (Engine.predict_chain_pages: units of same-shape pages, uploads, encoder and downloads of neighbouring
        units overlapped); each PNG stream is written to its file as it arrives.  Same files, names and bytes as write_masks.  Pages
        the device path cannot take -- other extensions than ".png", output.DEVICE_PNG = False, a foreign post-processor, more than
        256 classes, no binarisation where one is needed, a page the whole-page path would refuse (write_masks predicts it in
        tiles) -- go through write_masks, in place.  Yields the three paths per page, in
        dataset order.  mixed: True forms the units from the pages of one canvas whatever their shapes (chain_units_mixed; same
        bytes), False from runs of same-shape pages; None: MIXED_DEFAULT where the device pages of a chunk have more than one
        distinct (H, W, final H, final W) -- a one-shape chunk always takes the same-shape path."""
        from . import output
        level = output.DEVICE_PNG_LEVEL if level is None else level
        output_dir = output_dir if output_dir is not None else self.settings.output
        if output_dir is None:
            raise Exception("write_masks needs an output directory")
        for sub in ("color", "overlay", "inverted"):
            os.makedirs(os.path.join(output_dir, sub), exist_ok=True)
        pages = list(dataset.data)
        names = ("color", "overlay", "inverted")
        for i in range(0, len(pages), max(1, int(chunk_pages))):
            chunk = pages[i:i + max(1, int(chunk_pages))]
            paths, inputs = [], []
            for data in chunk:
                p = output.output_paths(output_dir, data)
                paths.append(p)
                inputs.append(self._chain_inputs(data, "png", record=False) if output.DEVICE_PNG and output.is_png_target(p[0]) else None)
                if inputs[-1] is not None and not self._list_takes(np.shape(inputs[-1][1])[:2]):
                    inputs[-1] = None
            on_device = [k for k, got in enumerate(inputs) if got is not None]
            if on_device:
                def to_file(page, name, stream, paths=paths, on_device=on_device):
                    with open(paths[on_device[page]][names.index(name)], "wb") as f:
                        f.write(stream)
                shapes = set((tuple(np.shape(inputs[k][1])[:2]), inputs[k][3] or tuple(np.shape(inputs[k][1])[:2])) for k in on_device)
                use_mixed = (self.MIXED_DEFAULT and len(shapes) > 1) if mixed is None else bool(mixed)
                self.network.model.predict_chain_pages(
                    [inputs[k][1] for k in on_device], binaries=[inputs[k][2] for k in on_device],
                    out_shapes=[inputs[k][3] for k in on_device], post_ops=inputs[on_device[0]][4],
                    exact_labels=self.network.exact == "labels", lut=self.settings.color_map.lut(), which=names,
                    png_level=level, sink=to_file, mixed=use_mixed)
            for k, data in enumerate(chunk):
                if inputs[k] is None:
                    self.write_masks(data, output_dir=output_dir, level=level)
                yield paths[k]

    def evaluate_dataset(self, dataset: Dataset, rules=(), connectivity=4, chunk=64, mixed=None):
        """Every page of a dataset predicted and scored against its mask: one evaluation.PageScore per page, in dataset order.
        Per chunk of `chunk` pages the list chain (Engine.predict_chain_pages with which=(), labels=True; the settings'
        post-processors and high_res_output, prepared as write_masks_dataset prepares them) hands down the uint8 label maps, and
        ONE evaluation.evaluate_pages call scores them against data.mask and the binarisation the chain used.  Pages the list
        chain cannot take (_chain_inputs, _list_takes) go through predict_single.  rules / connectivity: evaluate_pages'.
        mixed: write_masks_dataset's.  A page without a mask, or whose mask has not the shape of the final label map, raises
        and names the entry."""
        from .evaluation import evaluate_pages
        pages = list(dataset.data)
        name = lambda k, data: "entry %d (%s)" % (k, data.image_path or data.mask_path or "unnamed")
        for k, data in enumerate(pages):
            if data.mask is None:
                raise Exception("evaluate_dataset: %s has no mask" % name(k, data))
        scores = []
        step = max(1, int(chunk))
        for i in range(0, len(pages), step):
            part = pages[i:i + step]
            inputs = []
            for data in part:
                inputs.append(self._chain_inputs(data, True, record=False))
                if inputs[-1] is not None and not self._list_takes(np.shape(inputs[-1][1])[:2]):
                    inputs[-1] = None
            labels, binaries = [None] * len(part), [None] * len(part)
            on_device = [k for k, got in enumerate(inputs) if got is not None]
            if on_device:
                shapes = set((tuple(np.shape(inputs[k][1])[:2]), inputs[k][3] or tuple(np.shape(inputs[k][1])[:2])) for k in on_device)
                use_mixed = (self.MIXED_DEFAULT and len(shapes) > 1) if mixed is None else bool(mixed)
                got = self.network.model.predict_chain_pages(
                    [inputs[k][1] for k in on_device], binaries=[inputs[k][2] for k in on_device],
                    out_shapes=[inputs[k][3] for k in on_device], post_ops=inputs[on_device[0]][4],
                    exact_labels=self.network.exact == "labels", which=(), labels=True, mixed=use_mixed)
                for j, k in enumerate(on_device):
                    labels[k], binaries[k] = got[j]["labels"], inputs[k][2]
            for k, data in enumerate(part):
                if inputs[k] is None:
                    pred = self.predict_single(data)
                    labels[k] = np.asarray(pred.labels)
                    binaries[k] = None if pred.data.binary is None else np.asarray(pred.data.binary)
                if np.shape(data.mask) != np.shape(labels[k]):
                    raise Exception("evaluate_dataset: %s: the mask has shape %r, the label map %r"
                                    % (name(i + k, data), np.shape(data.mask), np.shape(labels[k])))
            scores += evaluate_pages([data.mask for data in part], labels, binaries, rules, connectivity)
        return scores

    #: predict_regions' route when none is given: "list" until the chain route has been measured against it (README, text regions)
    REGIONS_ROUTE_DEFAULT = "list"

    def predict_regions(self, dataset: Dataset, label, chunk=64, route=None):
        """The text regions of every page of a dataset: one list of pc_segmentation.TextRegion per page, in dataset order.  Per
        chunk of `chunk` pages the label maps come from the list route evaluate_dataset uses (the settings' post-processors and
        high_res_output; pages it cannot take go through predict_single), at their final shape, and ONE pseg_amd.text_regions call
        turns them into masks and region tables; the polygons are traced on the host.  label: the label id, or a ColorMap (its
        label named "text").  A page's char_height is its line_height_px at the scale of its label map.
        route: "list" is the above; "chain" makes ONE chain call per chunk with the regions stage (Engine.predict_chain_pages with
        which=(), labels=False, regions=...): the label maps never leave the device, the regions and their polygons come back.  A
        page whose record has a non-zero status, or one the list chain cannot take, goes through the list route, in place and in
        order.  None: REGIONS_ROUTE_DEFAULT.  Both routes give the same regions."""
        from pseg_amd import engine
        from .pc_segmentation import _label_of, regions_of_record
        route = self.REGIONS_ROUTE_DEFAULT if route is None else route
        if route not in ("chain", "list"):
            raise Exception("predict_regions: route must be 'chain' or 'list', got %r" % (route,))
        lid = _label_of(label)
        pages = list(dataset.data)
        out = []
        step = max(1, int(chunk))

        def height(data, final_h):
            ch = data.line_height_px or 1
            if data.original_shape is not None and data.original_shape[0]:
                ch = ch * final_h / data.original_shape[0]
            return ch
        for i in range(0, len(pages), step):
            part = pages[i:i + step]
            inputs = []
            for data in part:
                inputs.append(self._chain_inputs(data, False, record=False))
                if inputs[-1] is not None and not self._list_takes(np.shape(inputs[-1][1])[:2]):
                    inputs[-1] = None
            labels = [None] * len(part)
            done = [None] * len(part)
            on_device = [k for k, got in enumerate(inputs) if got is not None]
            if on_device and route == "chain":
                shapes = set((tuple(np.shape(inputs[k][1])[:2]), inputs[k][3] or tuple(np.shape(inputs[k][1])[:2])) for k in on_device)
                hows = [engine.TextRegions(lid, char_height=height(part[k], (inputs[k][3] or np.shape(inputs[k][1]))[0])) for k in on_device]
                got = self.network.model.predict_chain_pages(
                    [inputs[k][1] for k in on_device], binaries=[inputs[k][2] for k in on_device],
                    out_shapes=[inputs[k][3] for k in on_device], post_ops=inputs[on_device[0]][4],
                    exact_labels=self.network.exact == "labels", which=(), labels=False, mixed=self.MIXED_DEFAULT and len(shapes) > 1,
                    regions=hows)
                for j, k in enumerate(on_device):
                    if got[j]["regions"]["status"] == 0:
                        done[k] = regions_of_record(got[j]["regions"])
                on_device = [k for k in on_device if done[k] is None]
            if on_device:
                shapes = set((tuple(np.shape(inputs[k][1])[:2]), inputs[k][3] or tuple(np.shape(inputs[k][1])[:2])) for k in on_device)
                got = self.network.model.predict_chain_pages(
                    [inputs[k][1] for k in on_device], binaries=[inputs[k][2] for k in on_device],
                    out_shapes=[inputs[k][3] for k in on_device], post_ops=inputs[on_device[0]][4],
                    exact_labels=self.network.exact == "labels", which=(), labels=True, mixed=self.MIXED_DEFAULT and len(shapes) > 1)
                for j, k in enumerate(on_device):
                    labels[k] = got[j]["labels"]
            how, rest = [], [k for k in range(len(part)) if done[k] is None]
            for k in rest:
                if inputs[k] is None:
                    labels[k] = np.asarray(self.predict_single(part[k]).labels).astype(np.uint8)
                how.append(engine.TextRegions(lid, char_height=height(part[k], np.shape(labels[k])[0])))
            if rest:
                for k, rec in zip(rest, engine.text_regions([labels[k] for k in rest], how)):
                    done[k] = regions_of_record(rec)
            out += done
        return out

    def _scan_route(self, entry: SingleData, path):
        """Whether write_masks_scans may send this entry through the scan chain, as far as that shows before the file is read."""
        from . import output
        net = self.network
        return (entry.image is None and entry.image_path is not None and output.DEVICE_PNG and output.is_png_target(path)
                and self._chain_ops() is not None and net.n_classes <= 256 and not getattr(net, "_rgb", False))

    def write_masks_scans(self, entries, loader, output_dir=None, level=None, chunk_pages=64, decode_threads=2, decode="host", binarize=None,
                          despeckle=None, regions=None, on_regions=None, deskew=None, on_skew=None):
        """loader.load_images + write_masks_dataset for entries that name their scan by image_path, without the normalised page, the
        binarisation or the label map visiting the host: the decoded gray scans go through Engine.predict_chain_scans chunk_pages at
        a time (binarisation and line-height normalisation on the device, then the page chain), and each PNG stream is written to
        its file as it arrives.  Same files, names and bytes as that pair of calls; settings.high_res_output as there.  loader: a
        DatasetLoader, read for target_line_height and max_width.  While the device call of one chunk runs, decode_threads threads
        decode the files of the next one (dataset._imread_gray; the call releases the GIL).  Entries the scan chain cannot take -- a
        pre-loaded entry.image, a max_width that brings the second stage, another extension than ".png", output.DEVICE_PNG = False,
        a foreign post-processor, an rgb network, more than 256 classes, a page the whole-page path would refuse -- go through
        loader.load_images + write_masks, in place;
        the others are not modified.  Yields the three paths per entry, in order; a file that cannot be decoded raises when its
        entry is reached, after the paths of the entries in front of it.
        An entry whose line_height_px is None is measured here: once a chunk's files are decoded, the scans of such entries go
        through engine.char_heights(inverse=False) in ONE device call (compute_char_height's value, without a second decode), and
        the height is stored into entry.line_height_px -- the entry is modified, as the reference's loader modifies its records.
        It gives the scale on both routes, the scan chain and the fallback.  A scan without a measurable height (no glyph-shaped
        component) raises Exception naming the file when its entry is reached, as a file that cannot be decoded does.
        decode="device": the pool threads only read the files' bytes, and ONE pool task per chunk decodes them on the device
        (engine.png_decode_gray, 8-bit gray and RGB PNG files) -- on the decoder's own stream and workspace, while the calling
        thread runs the chain of the chunk before.  A file the decoder does not take or refuses is read with
        dataset._imread_gray, as under "host": its array, or its exception when the entry is reached, is PIL's.  Same files and
        bytes as decode="host".
        binarize: None (ink = scan <= 127) or a pseg_amd.Sauvola: the adaptive ink map, made on the device inside the chain, is what
        the vote and the masks work on -- the files of DatasetLoader(binarize=...).load_images + write_masks_dataset.  A window=None
        takes pseg_amd.sauvola_window of the entry's line height, the measured one for entries measured here; the fallback route
        loads the entry with the same binarisation.
        despeckle: None or a pseg_amd.Despeckle: the ink map (of either threshold) loses every component of at most max_area pixels
        on the device inside the chain, in front of the sampler -- the files of DatasetLoader(despeckle=...).load_images +
        write_masks_dataset.  A max_area=None takes pseg_amd.despeckle_area of the entry's line height, the measured one for
        entries measured here; the fallback route loads the entry with the same despeckling.
        regions: None, or a label id or a ColorMap (its label named "text"): the chain call gets the regions stage
        (Engine.predict_chain_scans(regions=...)), so a book goes from files to mask files and region polygons in one pass, and
        on_regions(entry_index, [TextRegion]) is called for every entry, in order, before its paths are yielded.  The regions are
        predict_regions' for the loaded entry: char_height is the entry's line_height_px at the scale of its label map, the
        measured height for entries measured here.  The mask files are those of the call without `regions`.  A page whose record
        comes back with a non-zero status, and every entry on the fallback route, gets its regions from predict_regions(route="list")
        on the loaded entry.
        deskew: None or a pseg_amd.Skew: after a chunk's scans are decoded and its missing line heights measured (on the scans as
        decoded), ONE pseg_amd.deskew_scans call per chunk replaces the arrays of the entries on the scan route by their deskewed
        scans (skew estimated on scan <= 127, rotation order 1, fill 255); the fallback route loads the entry with the same
        deskew.  on_skew(entry_index, index, denom) is called for every deskewed entry, in order, before its paths are yielded (a
        pre-loaded entry.image is not deskewed and gets no call).  The mask files are those of DatasetLoader(deskew=...).load_images
        + write_masks_dataset.  THE MASKS (and regions) ARE IN THE DESKEWED FRAME: a mask decoded to an array goes back to the
        scan's frame with pseg_amd.rotate_maps([mask], -index, denom) (order 0)."""
        if (regions is None) != (on_regions is None):
            raise Exception("write_masks_scans: regions and on_regions go together")
        if decode not in ("host", "device"):
            raise Exception(f"decode must be 'host' or 'device', got {decode!r}")
        from .dataset import check_binarize, check_despeckle, check_deskew, check_on_skew
        check_binarize(binarize)
        check_despeckle(despeckle)
        check_deskew(deskew)
        check_on_skew(deskew, on_skew)
        from concurrent.futures import ThreadPoolExecutor
        from pseg_amd import engine as _eng
        from . import dataset as _ds
        from . import output
        from .pc_segmentation import _label_of, regions_of_record
        lid = None if regions is None else _label_of(regions)
        level = output.DEVICE_PNG_LEVEL if level is None else level
        output_dir = output_dir if output_dir is not None else self.settings.output
        if output_dir is None:
            raise Exception("write_masks needs an output directory")
        for sub in ("color", "overlay", "inverted"):
            os.makedirs(os.path.join(output_dir, sub), exist_ok=True)
        entries = list(entries)
        step = max(1, int(chunk_pages))
        names = ("color", "overlay", "inverted")
        high_res = bool(self.settings.high_res_output)

        def load(entry, skews=None, k=None):
            """The entry as the fallback route loads it (the caller's entry is not modified)."""
            if deskew is not None:
                def note(_, index, denom):
                    if skews is not None:
                        skews[k] = index
                return loader._load_images(entry, binarize if binarize is not None else getattr(loader, "binarize", None),
                                           despeckle if despeckle is not None else getattr(loader, "despeckle", None), deskew, note)
            if despeckle is not None:
                return loader._load_images(entry, binarize if binarize is not None else getattr(loader, "binarize", None), despeckle)
            return loader.load_images(entry) if binarize is None else loader._load_images(entry, binarize)

        def regions_of_loaded(loaded):
            return self.predict_regions(Dataset([loaded], self.settings.color_map), lid, route="list")[0]

        def decode_entry(entry):
            return np.ascontiguousarray(_ds._imread_gray(entry.image_path), dtype=np.uint8)

        class _OfChunk:
            """One file's share of a chunk's decode task, with a future's result()."""
            def __init__(self, fut, k):
                self.fut, self.k = fut, k

            def result(self):
                r = self.fut.result()[self.k]
                if isinstance(r, BaseException):
                    raise r
                return r

        device = getattr(self.network.model, "device", 0)

        with ThreadPoolExecutor(max(1, int(decode_threads))) as pool:
            def start(i):
                """Chunk i's paths and the decodes of its device candidates, in flight."""
                chunk = entries[i:i + step]
                paths = [output.output_paths(output_dir, e) for e in chunk]
                wanted = [self._scan_route(e, p[0]) or (e.line_height_px is None and e.image_path is not None) for e, p in zip(chunk, paths)]
                if decode == "device":
                    ks = [k for k, w in enumerate(wanted) if w]
                    reads = [pool.submit(_eng.read_file_bytes, chunk[k].image_path) for k in ks]
                    fut = pool.submit(_eng.decode_gray_files, [chunk[k].image_path for k in ks], device, _ds._imread_gray, reads) if ks else None
                    slot = {k: j for j, k in enumerate(ks)}
                    return chunk, paths, [_OfChunk(fut, slot[k]) if w else None for k, w in enumerate(wanted)]
                return chunk, paths, [pool.submit(decode_entry, e) if w else None for e, w in zip(chunk, wanted)]

            ahead = start(0) if entries else None
            for i in range(0, len(entries), step):
                chunk, paths, pending = ahead
                ahead = start(i + step) if i + step < len(entries) else None
                scans, failed = [None] * len(chunk), None
                decoded = [None] * len(chunk)
                for k, fut in enumerate(pending):
                    if fut is None:
                        continue
                    try:
                        decoded[k] = fut.result()
                    except BaseException as exc:
                        failed = (k, exc)
                        break
                # the entries without a line height: one device call over the chunk's scans (a pre-loaded image is measured as it is)
                unmeasured = [k for k in range(len(chunk) if failed is None else failed[0]) if chunk[k].line_height_px is None]
                if unmeasured:
                    grays = [decoded[k] if decoded[k] is not None else np.ascontiguousarray(chunk[k].image, dtype=np.uint8) for k in unmeasured]
                    for k, h in zip(unmeasured, _eng.char_heights(grays, inverse=False)[0]):
                        if h is None:
                            if failed is None or k < failed[0]:
                                failed = (k, Exception(f"No line height could be measured in {chunk[k].image_path}"))
                        else:
                            chunk[k].line_height_px = h
                for k, scan in enumerate(decoded):
                    if scan is None or (failed is not None and k >= failed[0]) or not self._scan_route(chunk[k], paths[k][0]):
                        continue
                    scale = loader.target_line_height / chunk[k].line_height_px
                    # (the max_width stage shows only once the scan's shape is known)
                    page_shape = _eng.rescale_shape(scan.shape, scale)
                    if (loader.max_width is None or loader.max_width / page_shape[1] >= 1.0) and self._list_takes(page_shape):
                        scans[k] = (scan, scale)
                stop = len(chunk) if failed is None else failed[0]
                on_device = [k for k in range(stop) if scans[k] is not None]
                found = [None] * len(chunk)
                skews = [None] * len(chunk)
                if on_device and deskew is not None:       # one list call per chunk: the scan-route entries' arrays, deskewed
                    turned, idx = _eng.deskew_scans([scans[k][0] for k in on_device], deskew, device=device)
                    for k, t, a in zip(on_device, turned, idx):
                        scans[k], skews[k] = (t, scans[k][1]), int(a)
                if on_device:
                    def to_file(page, name, stream, paths=paths, on_device=on_device, found=found):
                        if name == "regions":
                            if stream["status"] == 0:
                                found[on_device[page]] = regions_of_record(stream)
                            return
                        with open(paths[on_device[page]][names.index(name)], "wb") as f:
                            f.write(stream)
                    # (the keyword goes only with a binarisation: today's call is unchanged)
                    how = {} if binarize is None else {"binarize": [binarize.resolved(chunk[k].line_height_px) for k in on_device]}
                    if despeckle is not None:
                        how["despeckle"] = [despeckle.resolved(chunk[k].line_height_px) for k in on_device]
                    if lid is not None:                    # predict_regions' rule: the line height at the scale of the label map
                        final_h = [scans[k][0].shape[0] if high_res else _eng.rescale_shape(scans[k][0].shape, scans[k][1])[0] for k in on_device]
                        how["regions"] = [_eng.TextRegions(lid, char_height=chunk[k].line_height_px * fh / scans[k][0].shape[0])
                                          for k, fh in zip(on_device, final_h)]
                    self.network.model.predict_chain_scans(
                        [scans[k][0] for k in on_device], [scans[k][1] for k in on_device], high_res=high_res,
                        post_ops=self._chain_ops(), exact_labels=self.network.exact == "labels", lut=self.settings.color_map.lut(),
                        which=names, png_level=level, sink=to_file, **how)
                for k in range(stop):
                    loaded = None
                    if scans[k] is None:
                        loaded = load(chunk[k], skews, k)
                        self.write_masks(loaded, output_dir=output_dir, level=level)
                    if on_skew is not None and skews[k] is not None:
                        on_skew(i + k, skews[k], deskew.denom)
                    if lid is not None:
                        if found[k] is None:
                            found[k] = regions_of_loaded(loaded if loaded is not None else load(dataclasses.replace(chunk[k])))
                        on_regions(i + k, found[k])
                    yield paths[k]
                if failed is not None:
                    raise failed[1]
