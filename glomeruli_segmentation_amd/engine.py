"""Host-side owner of a ``gs_espnet`` handle: packs a reference state_dict into the weight blob
the C ABI takes and exposes the hot-path calls on torch HIP tensors.

torch is used for device memory and streams only; all arithmetic happens in libglomseg.so.
"""
import ctypes
import functools

import numpy as np
import torch

from . import _call, _lib


def _to_numpy(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def pack_state_dict(state_dict):
    """state_dict (name -> tensor/array) -> (fp32 blob, LayerDesc array).  Integer buffers such as
    BatchNorm's num_batches_tracked are not arithmetic inputs and are skipped.
    Replaces torch.load + load_state_dict at VisualizeResults_iou.py:272,279."""
    items = []
    total = 0
    for name, v in state_dict.items():
        a = _to_numpy(v)
        if a.dtype.kind != "f":
            continue
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim > 4:
            raise ValueError("tensor %s has %d dims" % (name, a.ndim))
        items.append((name, a, total))
        total += a.size
    blob = np.empty(total, dtype=np.float32)
    table = (_lib.LayerDesc * len(items))()
    for i, (name, a, off) in enumerate(items):
        blob[off:off + a.size] = a.ravel()
        enc = name.encode()
        if len(enc) >= 96:
            raise ValueError("tensor name too long: " + name)
        table[i].name = enc
        table[i].offset = off
        table[i].ndim = a.ndim
        for d in range(a.ndim):
            table[i].shape[d] = a.shape[d]
    return blob, table


def _check_out(t, name, shape, dtype, device):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or \
            t.device.type != torch.device(device).type or (t.is_cuda and t.device != torch.device(device)):
        raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), device))


class EspnetEngine:
    """One model on one GPU.  ``encoder_only`` builds ESPNet-C (keys without the 'encoder.' prefix)."""

    def __init__(self, state_dict, classes=5, p=2, q=8, encoder_only=False, device=None, lanes=1):
        if not torch.cuda.is_available():
            raise RuntimeError("EspnetEngine needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU path in this build")
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        self.classes, self.p, self.q, self.encoder_only = classes, p, q, encoder_only
        blob, table = pack_state_dict(state_dict)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_espnet_create(blob.ctypes.data_as(ctypes.c_void_p), table, len(table), classes, p,
                                                 q, 1 if encoder_only else 0, ctypes.byref(h)))
        self.handle = h
        # lanes: extra activation workspaces (weights shared) so that several batches are in flight, each on a stream of
        # its own -- the tail of one batch's kernels overlaps the head of another's (include/glomseg.h, "LANES")
        self.lanes = 1
        self._lane_streams = {}
        if lanes != 1:
            self.set_lanes(lanes)

    def set_lanes(self, n):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_espnet_set_lanes(self.handle, int(n)))
        self.lanes = int(n)

    def lane_stream(self, lane):
        """the torch stream lane `lane` runs on (created on first use)"""
        if not 0 <= lane < self.lanes:
            raise ValueError("lane %d of %d" % (lane, self.lanes))
        if lane not in self._lane_streams:
            self._lane_streams[lane] = torch.cuda.Stream(device=self.device)
        return self._lane_streams[lane]

    def wait_lanes(self):
        """make the current stream wait for everything submitted to the lanes (their outputs are then safe to use on it)"""
        cur = torch.cuda.current_stream(self.device)
        for st in self._lane_streams.values():
            cur.wait_stream(st)

    def quiesce(self):
        """block until everything submitted for this handle -- on the current stream or on a lane's stream -- has finished.
        The host pipelines (segment_host, segment_crops) run on streams of the library's own in workspaces 0 and 1 and
        expect exactly that (include/glomseg.h)."""
        for st in self._lane_streams.values():
            st.synchronize()
        torch.cuda.current_stream(self.device).synchronize()

    def check_device_faults(self):
        """Synchronise the device and raise if a kernel of an earlier stream-ordered call (segment / forward_logits / lanes) reported
        through the device-side fault word that it went on without data it was waiting for (gs_device_fault_check; the host
        pipelines check by themselves).  Cheap: one device synchronise and a 4-byte read."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_device_fault_check())

    def close(self):
        if getattr(self, "handle", None):
            with torch.cuda.device(self.device):
                self.lib.gs_espnet_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ hot path
    def _lane_call(self, lane, tensors):
        """(workspace index, stream pointer) for a stream-ordered call that uses `tensors` (all on one device; None entries are
        skipped).  lane=None: workspace 0 on the current stream.  lane=k: workspace k on that lane's own stream, which first waits
        for the current one."""
        dev = tensors[0].device
        if lane is None:
            if 0 in self._lane_streams:      # workspace 0 may still be in use on lane 0's own stream
                torch.cuda.current_stream(dev).wait_stream(self._lane_streams[0])
            return 0, _call.stream_ptr(dev)
        st = self.lane_stream(lane)
        st.wait_stream(torch.cuda.current_stream(dev))
        for t in tensors:      # (allocator: these tensors are in use on the lane's stream)
            if t is not None:
                t.record_stream(st)
        return lane, ctypes.c_void_p(st.cuda_stream)

    def reserve(self, n, height, width):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_espnet_reserve(self.handle, n, height, width))

    def forward_logits(self, x):
        """fp32 [N,3,H,W] on the GPU -> logits [N,classes,H,W] ([N,classes,H/8,W/8] for ESPNet-C).
        The nn.Module.forward replacement (Model.py:341 / :273)."""
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_cuda:
            raise ValueError("expected a float32 [N,3,H,W] tensor on the GPU")
        x = x.contiguous()
        n, _, h, w = x.shape
        oh, ow = (h // 8, w // 8) if self.encoder_only else (h, w)
        out = torch.empty((n, self.classes, oh, ow), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(self.lib.gs_espnet_forward(self.handle, x.data_ptr(), _lib.GS_IN_F32_NCHW, n, h, w, None, None,
                                                  out.data_ptr(), None, None, _call.stream_ptr(x.device)))
        return out

    def segment(self, tiles_u8, mean, std, want_logits=False, want_hist=True, out_mask=None, out_hist=None, lane=None,
                want_enc_logits=False):
        """uint8 BGR [N,H,W,3] on the GPU -> (mask uint8 [N,H,W], counts int64 [N,classes], logits|None).
        One pass of VisualizeResults_iou.py:107-128,151-155 for a batch.
        ESPNet-C (encoder_only): the mask is the argmax of the encoder's logits upsampled x8 (:125-126,258-261), from the
        library's head kernel; want_enc_logits=True also returns the 1/8-scale logits [N,classes,H/8,W/8] the mask of the SAME
        pass was computed from (want_logits is refused for such an engine: it has no full-resolution logits).
        lane=None: on the current stream, in workspace 0.  lane=k: in workspace k on that lane's own stream (which first
        waits for the current stream, so inputs produced there are ready); the outputs belong to the lane's stream until
        wait_lanes() -- submit the next batch to another lane meanwhile."""
        if tiles_u8.dtype != torch.uint8 or tiles_u8.dim() != 4 or tiles_u8.shape[3] != 3 or not tiles_u8.is_cuda:
            raise ValueError("expected a uint8 [N,H,W,3] tensor on the GPU")
        if want_enc_logits and not self.encoder_only:
            raise ValueError("want_enc_logits: the 1/8-scale logits are an output of ESPNet-C engines only")
        if want_logits and self.encoder_only:
            raise ValueError("want_logits: an ESPNet-C engine has no full-resolution logits (want_enc_logits=True gives the 1/8-scale ones)")
        want_logits = bool(want_logits or want_enc_logits)
        tiles_u8 = tiles_u8.contiguous()
        n, h, w, _ = tiles_u8.shape
        dev = tiles_u8.device
        # caller-supplied outputs are written by the kernels as plain pointers: refuse anything that is not exactly the
        # buffer the call would have allocated itself
        _check_out(out_mask, "out_mask", (n, h, w), torch.uint8, dev)
        _check_out(out_hist, "out_hist", (n, self.classes), torch.int64, dev)
        mask = out_mask if out_mask is not None else torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        hist = None
        if want_hist:
            hist = out_hist if out_hist is not None else torch.empty((n, self.classes), dtype=torch.int64, device=dev)
        lh, lw = (h // 8, w // 8) if self.encoder_only else (h, w)
        logits = torch.empty((n, self.classes, lh, lw), dtype=torch.float32, device=dev) if want_logits else None
        with torch.cuda.device(dev):
            k, sp = self._lane_call(lane, (tiles_u8, mask, hist, logits))
            _lib.check(self.lib.gs_espnet_forward_lane(
                self.handle, k, tiles_u8.data_ptr(), _lib.GS_IN_U8_BGR_NHWC, n, h, w, _lib.fptr3(mean), _lib.fptr3(std),
                logits.data_ptr() if want_logits else None, mask.data_ptr(),
                hist.data_ptr() if want_hist else None, sp))
        return mask, hist, logits

    def segment_host(self, tiles, mean, std, batch=32, want_hist=True, out_masks=None, out_hist=None):
        """numpy uint8 [T,H,W,3] in host memory -> (masks [T,H,W], counts [T,classes]) through the
        pinned double-buffered H2D / compute / D2H pipeline of the library."""
        self.quiesce()
        from_tensor = isinstance(tiles, torch.Tensor)
        if from_tensor:      # e.g. a pinned CPU tensor: DMA'd in place, no staging copy; the outputs are tensors pinned like it
            if tiles.is_cuda or tiles.dtype != torch.uint8 or not tiles.is_contiguous():
                raise ValueError("expected a contiguous uint8 CPU tensor")
            t, h, w, _ = tiles.shape
            pin = tiles.is_pinned()
            _check_out(out_masks, "out_masks", (t, h, w), torch.uint8, torch.device("cpu"))
            _check_out(out_hist, "out_hist", (t, self.classes), torch.int64, torch.device("cpu"))
            masks = out_masks if out_masks is not None else torch.empty((t, h, w), dtype=torch.uint8, pin_memory=pin)
            hist = None
            if want_hist:
                hist = out_hist if out_hist is not None else torch.zeros((t, self.classes), dtype=torch.int64, pin_memory=pin)
            in_ptr, mask_ptr, hist_ptr = tiles.data_ptr(), masks.data_ptr(), hist.data_ptr() if want_hist else None
        else:
            tiles = np.ascontiguousarray(tiles, dtype=np.uint8)
            t, h, w, _ = tiles.shape
            masks = np.empty((t, h, w), dtype=np.uint8)
            hist = np.zeros((t, self.classes), dtype=np.uint64) if want_hist else None
            in_ptr, mask_ptr, hist_ptr = tiles.ctypes.data, masks.ctypes.data, hist.ctypes.data if want_hist else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_espnet_segment_host(
                self.handle, ctypes.c_void_p(in_ptr), t, h, w, _lib.fptr3(mean), _lib.fptr3(std), batch, ctypes.c_void_p(mask_ptr),
                ctypes.c_void_p(hist_ptr)))
        if from_tensor:
            return masks.numpy(), (hist.numpy() if want_hist else None)
        return masks, (hist.astype(np.int64) if want_hist else None)

    scores_crops = True      # segment_crops takes labels= / want_gt_overlay= (segment.segment_batch asks)

    def segment_crops(self, crops, mean, std, net_h=512, net_w=1024, batch=32, **kw):
        """The loop of VisualizeResults_iou.py:100-156 over crops of ANY sizes (numpy uint8 BGR [h,w,3] each, or pinned CPU
        tensors) through the library's batched pipeline; see segment_crops_host for the keywords and the result."""
        return segment_crops_host([self], [(mean, std)], crops, net_h, net_w, batch, **kw)

    def segment_crops_resident(self, packed_in, descs, mean, std, net_h=512, net_w=1024, want_net_maps=True, want_hist=True,
                               packed_out=None, paste=None, lane=None):
        """Device-resident form (gs_espnet_segment_crops): packed_in is a uint8 GPU tensor holding the crops at
        descs[i].in_off, descs a list of _lib.CropDesc.  Returns (net_maps [n,net_h,net_w] | None, counts [n,5] | None);
        crop-size maps are written into packed_out (uint8 GPU tensor) at descs[i].out_off when it is given."""
        n = len(descs)
        dev = packed_in.device
        tab = (_lib.CropDesc * n)(*descs)
        net = torch.empty((n, net_h, net_w), dtype=torch.uint8, device=dev) if want_net_maps else None
        hist = torch.empty((n, self.classes), dtype=torch.int64, device=dev) if want_hist else None
        with torch.cuda.device(dev):
            k, sp = self._lane_call(lane, (packed_in, packed_out, net, hist))
            _lib.check(self.lib.gs_espnet_segment_crops(
                self.handle, k, packed_in.data_ptr(), tab, n, _lib.fptr3(mean), _lib.fptr3(std), net_h, net_w,
                net.data_ptr() if net is not None else None, packed_out.data_ptr() if packed_out is not None else None,
                hist.data_ptr() if hist is not None else None, ctypes.byref(paste) if paste is not None else None, sp))
        return net, hist

    # ------------------------------------------------------------------ test / bench hooks
    def read_stage(self, name, image=0):
        dims = (ctypes.c_int * 3)()
        _lib.check(self.lib.gs_espnet_read_stage(self.handle, name.encode(), image, None, 0, ctypes.byref(dims)))
        out = np.empty(tuple(dims), dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_espnet_read_stage(self.handle, name.encode(), image,
                                                     out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(dims)))
        return out

    def block_forward(self, kind, level, index, x):
        """One block of the trunk on a host CHW fp32 array (test hook; kind 0 = ESP block, 1 = DownSamplerB)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        c, h, w = x.shape
        cout = 64 if level == 2 else 128
        out = np.empty((cout, h, w) if kind == 0 else (cout, h // 2, w // 2), dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_espnet_block_forward(self.handle, kind, level, index, x.ctypes.data_as(ctypes.c_void_p),
                                                        h, w, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def workspace_audit(self, lane=0):
        """Test tool (gs_espnet_workspace_audit, include/glomseg_workspace.h): waits for the device and reports the words of lane
        `lane`'s activation workspace that must be zero and are not -> {"must_be_zero": words looked at, "offenders": how many
        are not 0x00000000, "first": None | {"piece", "image", "plane", "row", "col", "bits"}}."""
        rep = _lib.WorkspaceReport()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_espnet_workspace_audit(self.handle, lane, ctypes.byref(rep)))
        return _workspace_report(rep)

    def workspace_poison(self, pattern=0x7fc00000, lane=0):
        """Test tool (gs_espnet_workspace_poison): overwrites every interior and free float of lane `lane`'s activation workspace
        with the 32-bit pattern (a quiet NaN by default) and leaves the words that must be zero as they are."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_espnet_workspace_poison(self.handle, lane, pattern))

    def profile(self, on):
        _lib.check(self.lib.gs_espnet_profile_enable(self.handle, 1 if on else 0))

    def profile_read(self):
        arr = (_lib.KernelTime * 32)()
        n = ctypes.c_int()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_espnet_profile_read(self.handle, arr, 32, ctypes.byref(n)))
        return [{"name": arr[i].name.decode(), "total_ms": arr[i].total_ms, "launches": arr[i].launches,
                 "flops_per_tile": arr[i].flops_per_tile} for i in range(n.value)]


@functools.lru_cache(maxsize=None)
def forward_forms():
    """The library's table of kernel forms: [(launch class name, [(form name, pixels per lane), ...]), ...] in the order of
    the form codes (gs_espnet_form_info), read once.  Host-only: needs no GPU."""
    lib = _lib.load()
    table = []
    name, ppl = ctypes.c_char_p(), ctypes.c_int()
    while lib.gs_espnet_form_info(len(table), _lib.GS_FORM_NONE, ctypes.byref(name), ctypes.byref(ppl)) == _lib.GS_OK:
        k, cls, forms = len(table), name.value.decode(), []
        while lib.gs_espnet_form_info(k, len(forms), ctypes.byref(name), ctypes.byref(ppl)) == _lib.GS_OK:
            forms.append((name.value.decode(), ppl.value))
        table.append((cls, tuple(forms)))
    return tuple(table)


def plan_forward(n, height, width, p, q, classes, num_cus):
    """{launch class name: form name}: what a forward of n tiles of height x width launches for ESPNet(classes, p, q) on a
    device with num_cus compute units (gs_espnet_plan_forward, the planner the forward itself calls); a class that model does
    not launch is left out.  Host-only: needs no GPU."""
    lib = _lib.load()
    table = forward_forms()
    codes, count = (ctypes.c_int * len(table))(), ctypes.c_int()
    _lib.check(lib.gs_espnet_plan_forward(n, height, width, p, q, classes, num_cus, codes, len(table), ctypes.byref(count)))
    return {cls: forms[codes[k]][0] for k, (cls, forms) in enumerate(table) if codes[k] != _lib.GS_FORM_NONE}


def _plan_flag_bits(n, height, width, p, q, classes, num_cus, encoder_only):
    flags = ctypes.c_int()
    _lib.check(_lib.load().gs_espnet_plan_flags(n, height, width, p, q, classes, int(bool(encoder_only)), num_cus, ctypes.byref(flags)))
    return flags.value


def plan_flags(n, height, width, p, q, classes, num_cus, encoder_only=False):
    """{"lazy_b2": bool, "l3c_in_reduce": bool}: the decisions of the same plan that are no form of a launch class
    (gs_espnet_plan_flags, include/glomseg_plan.h).  Host-only: needs no GPU."""
    bits = _plan_flag_bits(n, height, width, p, q, classes, num_cus, encoder_only)
    return {"lazy_b2": bool(bits & _lib.GS_PLAN_LAZY_B2), "l3c_in_reduce": bool(bits & _lib.GS_PLAN_L3C_IN_REDUCE)}


def plan_cls_in_l3(n, height, width, p, q, classes, num_cus, encoder_only=False):
    """Whether the same plan sums the encoder classifier in the epilogues of the level-3 down-sampler and of the last
    level-3 ESP block (GS_PLAN_CLS_IN_L3 of gs_espnet_plan_flags; dec1_sums_kernel then adds the partial planes in
    dec1_kernel's place).  Host-only: needs no GPU."""
    return bool(_plan_flag_bits(n, height, width, p, q, classes, num_cus, encoder_only) & _lib.GS_PLAN_CLS_IN_L3)


def plan_lean(n, height, width, p, q, classes, num_cus, encoder_only=False, want_logits=False):
    """Whether a forward of this shape and model is lean when asked for logits or not: no logits, and both decoder projections
    planned as side sums of their producers, so that the last level-3 launch stores no map and the stage "level3.<q-1>" does
    not exist afterwards (gs_espnet_plan_lean, include/glomseg_lean.h).  Host-only: needs no GPU."""
    lean = ctypes.c_int()
    _lib.check(_lib.load().gs_espnet_plan_lean(n, height, width, p, q, classes, int(bool(encoder_only)), num_cus, int(bool(want_logits)),
                                               ctypes.byref(lean)))
    return bool(lean.value)


def pack_weights(state_dict, classes=5, p=2, q=8, encoder_only=False):
    """(blob, pieces): the fp32 weight blob gs_espnet_create uploads for this model and {piece name: (float offset, floats)} of
    its pieces in order (gs_espnet_pack_weights, include/glomseg_plan.h).  Host-only: needs no GPU."""
    lib = _lib.load()
    src, table = pack_state_dict(state_dict)
    head = (src.ctypes.data_as(ctypes.c_void_p), table, len(table), classes, p, q, int(bool(encoder_only)))
    n, n_pieces = ctypes.c_size_t(), ctypes.c_int()
    _lib.check(lib.gs_espnet_pack_weights(*head, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n_pieces)))
    blob, pieces = np.empty(n.value, dtype=np.float32), (_lib.WeightPiece * n_pieces.value)()
    _lib.check(lib.gs_espnet_pack_weights(*head, blob.ctypes.data_as(ctypes.c_void_p), blob.size, ctypes.byref(n), pieces, len(pieces),
                                          ctypes.byref(n_pieces)))
    return blob, {pc.name.decode(): (pc.offset, pc.floats) for pc in pieces}


def workspace_bytes(n, height, width, p, q, classes, encoder_only=False):
    """The bytes of activation workspace EspnetEngine.reserve(n, height, width) allocates per lane for ESPNet(classes, p, q)
    (gs_espnet_workspace_plan); raises GlomsegError for a shape no forward takes.  Host-only: needs no GPU."""
    return _call.planned_bytes(_lib.load().gs_espnet_workspace_plan, n, height, width, p, q, classes, bool(encoder_only))


def _workspace_report(rep):
    first = None
    if rep.offenders:
        first = {"piece": rep.piece.decode(), "image": rep.image, "plane": rep.plane, "row": rep.row, "col": rep.col, "bits": rep.bits}
    return {"must_be_zero": rep.must_be_zero, "offenders": rep.offenders, "first": first}


def workspace_classes(ws_n, height, width, p, q, classes, encoder_only=False):
    """[(piece, class map)] of the activation workspace reserve(ws_n, height, width) lays out per lane, in allocation order:
    piece = {"name", "offset" (bytes), "own_words", "span_words", "padded", "C", "Cp", "H", "W", "pitch", "sc", "off"}, class map =
    uint8 [span_words] of _lib.GS_WS_FREE / GS_WS_INTERIOR / GS_WS_MUST_BE_ZERO (gs_espnet_workspace_classes,
    include/glomseg_workspace.h).  Host-only: needs no GPU."""
    lib = _lib.load()
    head = (ws_n, height, width, p, q, classes, int(bool(encoder_only)))
    count = ctypes.c_int()
    _lib.check(lib.gs_espnet_workspace_classes(*head, 0, None, None, 0, ctypes.byref(count)))
    out = []
    for i in range(count.value):
        info = _lib.WorkspacePiece()
        _lib.check(lib.gs_espnet_workspace_classes(*head, i, ctypes.byref(info), None, 0, None))
        cmap = np.empty(info.span_words, dtype=np.uint8)
        _lib.check(lib.gs_espnet_workspace_classes(*head, i, None, cmap.ctypes.data_as(ctypes.c_void_p), cmap.size, None))
        piece = {k: getattr(info, k) for k, _ in _lib.WorkspacePiece._fields_}
        piece["name"], piece["padded"] = info.name.decode(), bool(info.padded)
        out.append((piece, cmap))
    return out


def workspace_audit_host(copy, ws_n, height, width, p, q, classes, encoder_only=False):
    """The audit of EspnetEngine.workspace_audit over a host copy (uint32 or float32 array) of a whole workspace allocation
    (gs_espnet_workspace_audit_host).  Host-only: needs no GPU."""
    copy = np.ascontiguousarray(copy)
    rep = _lib.WorkspaceReport()
    _lib.check(_lib.load().gs_espnet_workspace_audit_host(ws_n, height, width, p, q, classes, int(bool(encoder_only)),
                                                          copy.ctypes.data_as(ctypes.c_void_p), copy.nbytes, ctypes.byref(rep)))
    return _workspace_report(rep)


def crop_preprocess(crop_u8, mean, std, out_h, out_w, out=None):
    """uint8 BGR crop [h,w,3] on the GPU -> normalised, bilinearly resized fp32 [3,out_h,out_w]
    (VisualizeResults_iou.py:107-116 for a crop that is not network-sized)."""
    lib = _lib.load()
    crop_u8 = crop_u8.contiguous()
    h, w, _ = crop_u8.shape
    if out is None:
        out = torch.empty((3, out_h, out_w), dtype=torch.float32, device=crop_u8.device)
    with torch.cuda.device(crop_u8.device):
        _lib.check(lib.gs_crop_preprocess(crop_u8.data_ptr(), h, w, _lib.fptr3(mean), _lib.fptr3(std), out_h, out_w,
                                          out.data_ptr(), _call.stream_ptr(crop_u8.device)))
    return out


def mask_resize_nearest(mask, out_h, out_w):
    """uint8 class map [h,w] on the GPU -> [out_h,out_w], cv2.INTER_NEAREST sampling (:129)."""
    lib = _lib.load()
    mask = mask.contiguous()
    h, w = mask.shape
    out = torch.empty((out_h, out_w), dtype=torch.uint8, device=mask.device)
    with torch.cuda.device(mask.device):
        _lib.check(lib.gs_mask_resize_nearest(mask.data_ptr(), h, w, out_h, out_w, out.data_ptr(), _call.stream_ptr(mask.device)))
    return out


def paste_target(slide_map, ds=8, luts=None):
    """_lib.PasteTarget for a uint8 [map_h,map_w] GPU tensor (the 1/ds slide map of composite.SlideCompositor)."""
    if slide_map.dtype != torch.uint8 or slide_map.dim() != 2 or not slide_map.is_cuda or not slide_map.is_contiguous():
        raise ValueError("slide_map must be a contiguous uint8 [map_h,map_w] tensor on the GPU")
    t = _lib.PasteTarget()
    t.slide_map = slide_map.data_ptr()
    t.map_h, t.map_w, t.ds = int(slide_map.shape[0]), int(slide_map.shape[1]), int(ds)
    t.sx_lut = luts[0].data_ptr() if luts is not None else None
    t.sy_lut = luts[1].data_ptr() if luts is not None else None
    return t


def seen_values(seen_words):
    """the sorted uint8 values of a 256-bit set as gs_espnet_score_crops writes it (uint64 [4], bit v of word v // 64): np.unique of
    the label the set was collected from"""
    bits = np.unpackbits(np.ascontiguousarray(seen_words, dtype="<u8").view(np.uint8), bitorder="little")
    return np.nonzero(bits)[0].astype(np.uint8)


def score_crops_resident(net_masks, packed_labels, descs, classes, want_seen=True):
    """Device-resident scoring stage (gs_espnet_score_crops), on the current stream: net_masks uint8 [n,net_h,net_w] and
    packed_labels (uint8, crop i's [h,w] label at descs[i].out_off) on the GPU, descs a list of _lib.CropDesc ->
    (conf int64 [n,classes,classes], rows = ground truth; seen int64 [n,4] bit sets | None), GPU tensors."""
    lib = _lib.load()
    n, net_h, net_w = (int(v) for v in net_masks.shape)
    if n != len(descs):
        raise ValueError("%d masks for %d descriptors" % (n, len(descs)))
    if net_masks.dtype != torch.uint8 or packed_labels.dtype != torch.uint8 or not net_masks.is_contiguous() or not packed_labels.is_contiguous():
        raise ValueError("expected contiguous uint8 GPU tensors")
    need = max(int(d.out_off) + int(d.h) * int(d.w) for d in descs)
    if packed_labels.numel() < need:
        raise ValueError("packed_labels holds %d bytes, the descriptors reach %d" % (packed_labels.numel(), need))
    dev = net_masks.device
    tab = (_lib.CropDesc * n)(*descs)
    conf = torch.empty((n, classes, classes), dtype=torch.int64, device=dev)
    seen = torch.empty((n, 4), dtype=torch.int64, device=dev) if want_seen else None
    with torch.cuda.device(dev):
        _lib.check(lib.gs_espnet_score_crops(net_masks.data_ptr(), packed_labels.data_ptr(), tab, n, net_h, net_w, classes,
                                             conf.data_ptr(), seen.data_ptr() if seen is not None else None, _call.stream_ptr(dev)))
    return conf, seen


def segment_crops_host(engines, mean_stds, crops, net_h=512, net_w=1024, batch=32, want_masks=True, want_net_maps=False,
                       want_hist=True, paste=None, origins=None, overlay=None, labels=None, want_gt_overlay=False):
    """gs_espnet_segment_crops_host: crops of any sizes in host memory -> per-crop class maps at crop size.

    engines: one EspnetEngine (the plain model) or several (the cfg-5 ensemble, each with its own (mean, std) in mean_stds):
    all full networks, or all `encoder_only` (ESPNet-C) engines -- at most _lib.GS_MAX_ENSEMBLE_C of those, each listed once; the
    library then runs the members' trunks and one head over their 1/8-scale logits.  A list that mixes the two raises GlomsegError.
    crops: list of uint8 BGR [h,w,3] numpy arrays / CPU tensors (pinned ones are DMA'd in place).
    paste: an _lib.PasteTarget (see paste_target) + origins [(x1, y1), ...]: the crops are also max-composited into the
    slide map on the GPU.
    overlay: (palette uint8 [k,3] RGB, wa, wb): also return every crop's class map coloured and blended over the crop,
    cv2.addWeighted(crop, wa, colour, wb, 0) (VisualizeResults_iou.py:139-146), computed on the GPU for the whole batch.
    Returns dict(masks=list of uint8 [h,w] numpy views of one pinned buffer | None, net_maps=uint8 [n,net_h,net_w] | None,
    counts=int64 [n,classes] counts of the crop-size maps | None, overlays=list of uint8 [h,w,3] BGR views | None).
    labels: one uint8 [h,w] numpy array per crop, of the crop's size: the batch is also SCORED on the GPU
    (gs_espnet_segment_crops_host_scored, VisualizeResults_iou.py:195-203): the dict gains conf (int64 [n,classes,classes]: the
    confusion matrix, rows = ground truth, of the network-resolution map and the label nearest-resized to the network size) and
    seen (list of sorted uint8 arrays: np.unique of that resized label); with want_gt_overlay (needs `overlay`) also gt_overlays,
    the label coloured and blended like the prediction (:218-222; a value beyond the palette takes its last row).  Without
    labels the three are None.
    """
    lib = _lib.load()
    n = len(crops)
    if labels is not None and len(labels) != n:
        raise ValueError("%d labels for %d crops" % (len(labels), n))
    if want_gt_overlay and (labels is None or overlay is None):
        raise ValueError("want_gt_overlay needs labels and overlay")
    if n == 0:
        return {"masks": [] if want_masks else None, "net_maps": None, "counts": None, "overlays": [] if overlay is not None else None,
                "conf": None, "seen": [] if labels is not None else None, "gt_overlays": [] if want_gt_overlay else None}
    ptrs, shapes, keep = _call.host_image_ptrs(crops, "crop")      # keep: the converted inputs, alive for the duration of the call
    hs, ws = (ctypes.c_int * n)(*[h for h, _ in shapes]), (ctypes.c_int * n)(*[w for _, w in shapes])
    eng0 = engines[0]
    handles = (ctypes.c_void_p * len(engines))(*[e.handle for e in engines])
    means, stds = _call.mean_std_arrays(mean_stds, len(engines))
    out_ptrs, out_buf, offs = None, None, None
    if want_masks:       # one pinned buffer for all maps: the library DMAs every map straight to its place
        out_buf, offs, out_ptrs = _call.packed_pinned([h * w for h, w in shapes])
    net = torch.empty((n, net_h, net_w), dtype=torch.uint8, pin_memory=True) if want_net_maps else None
    hist = torch.zeros((n, eng0.classes), dtype=torch.int64, pin_memory=True) if want_hist else None
    x1 = y1 = None
    if paste is not None:
        if origins is None or len(origins) != n:
            raise ValueError("paste needs one (x1, y1) level-0 origin per crop")
        x1 = (ctypes.c_int * n)(*[int(o[0]) for o in origins])
        y1 = (ctypes.c_int * n)(*[int(o[1]) for o in origins])
    ov, ov_buf, ov_offs, pal = None, None, None, None
    if overlay is not None:     # one pinned buffer laid out like the library's packed input: a batch's overlays leave in one DMA
        palette, wa, wb = overlay
        pal = np.ascontiguousarray(palette, dtype=np.uint8).reshape(-1, 3)
        ov_buf, ov_offs, ov_ptrs = _call.packed_pinned([h * w * 3 for h, w in shapes])
        ov = _lib.CropOverlay()
        ov.palette_rgb = pal.ctypes.data
        ov.n_colours = int(pal.shape[0])
        ov.wa, ov.wb = float(wa), float(wb)
        ov.out_bgr = ctypes.cast(ov_ptrs, ctypes.POINTER(ctypes.c_void_p))
        keep.append(ov_ptrs)
    sc, conf, seen, gt_buf = None, None, None, None
    if labels is not None:
        lab_ptrs = (ctypes.c_void_p * n)()
        for i, lb in enumerate(labels):
            if not isinstance(lb, np.ndarray) or lb.dtype != np.uint8 or lb.shape != shapes[i]:
                raise ValueError("label %d: expected a uint8 [%d,%d] array" % ((i,) + shapes[i]))
            lb = np.ascontiguousarray(lb)
            keep.append(lb)
            lab_ptrs[i] = lb.ctypes.data
        conf = np.zeros((n, eng0.classes, eng0.classes), dtype=np.uint64)
        seen = np.zeros((n, 4), dtype=np.uint64)
        sc = _lib.CropScoring()
        sc.labels = ctypes.cast(lab_ptrs, ctypes.POINTER(ctypes.c_void_p))
        sc.conf, sc.seen = conf.ctypes.data, seen.ctypes.data
        sc.gt_clamp = 1
        keep.append(lab_ptrs)
        if want_gt_overlay:     # laid out like the overlays
            gt_buf, _, gt_ptrs = _call.packed_pinned([h * w * 3 for h, w in shapes])
            sc.gt_overlay_bgr = ctypes.cast(gt_ptrs, ctypes.POINTER(ctypes.c_void_p))
            keep.append(gt_ptrs)
    for e in engines:
        e.quiesce()
    args = (handles, len(engines), ptrs, hs, ws, n, means, stds, net_h, net_w, batch, out_ptrs,
            ctypes.c_void_p(net.data_ptr()) if net is not None else None,
            ctypes.c_void_p(hist.data_ptr()) if hist is not None else None,
            ctypes.byref(paste) if paste is not None else None, x1, y1, ctypes.byref(ov) if ov is not None else None)
    with torch.cuda.device(eng0.device):
        if sc is None:
            _lib.check(lib.gs_espnet_segment_crops_host(*args))
        else:
            _lib.check(lib.gs_espnet_segment_crops_host_scored(*args, ctypes.byref(sc)))
    masks = _call.packed_views(out_buf, offs, shapes) if want_masks else None
    bgr_shapes = [(h, w, 3) for h, w in shapes]
    overlays = _call.packed_views(ov_buf, ov_offs, bgr_shapes) if ov is not None else None
    gt_overlays = _call.packed_views(gt_buf, ov_offs, bgr_shapes) if gt_buf is not None else None
    return {"masks": masks, "net_maps": net.numpy() if net is not None else None,
            "counts": hist.numpy() if hist is not None else None, "overlays": overlays,
            "conf": conf.astype(np.int64) if conf is not None else None,
            "seen": [seen_values(seen[i]) for i in range(n)] if seen is not None else None, "gt_overlays": gt_overlays}


def ensemble_segment(engines, tiles_u8, mean_stds):
    """cfg 5: mean over models of softmax(logits_k) (each model with its own mean/std) -> argmax mask,
    per-class counts.  The reference has no ensemble code; the definition is this build's.
    The engines are all full networks, or all `encoder_only` (ESPNet-C) engines: 1 .. _lib.GS_MAX_ENSEMBLE_C of them, each listed
    once -- softmax of every member's x8-upsampled 1/8-scale logits, mean, first-max argmax in one head launch behind the members'
    trunks.  A mixed list, differing class counts and a ninth ESPNet-C member raise GlomsegError."""
    lib = _lib.load()
    tiles_u8 = tiles_u8.contiguous()
    n, h, w, _ = tiles_u8.shape
    dev = tiles_u8.device
    handles = (ctypes.c_void_p * len(engines))(*[e.handle for e in engines])
    means, stds = _call.mean_std_arrays(mean_stds, len(engines))
    mask = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    hist = torch.empty((n, engines[0].classes), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gs_espnet_ensemble_forward(handles, len(engines), tiles_u8.data_ptr(), n, h, w, means, stds,
                                                  mask.data_ptr(), hist.data_ptr(), _call.stream_ptr(dev)))
    return mask, hist
