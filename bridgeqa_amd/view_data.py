"""Image views prepared where they are consumed: the raw RGB frames stay resident on the device as bytes, and a batch of network
inputs -- what the reference builds per sample on the host with a Pillow bicubic resize, ToTensor and Normalize and then collates,
pins and uploads as fp32 (lib/dataset.py:130-142, 340-341; utils/blip_utils.py:96-111) -- is one launch of csrc/view_prep.hip.

    store = ViewStore(frames, device)                                      # once: (H, W, 3) uint8 frames of any sizes
    batcher = ViewBatcher(store, size=480)                                 # fp32 (B, V, 3, 480, 480), the reference's "images"
    batch = batcher.prepare(view_index, out=stager.next_batch)             # per step, in place
    patches = ViewBatcher(store, 480, dtype=torch.bfloat16, layout="patches")   # what vit.PatchEmbed's GEMM reads, unfolded

The definition (Pillow's 8-bit resize, restated; tests/viewprep_ref.py holds it to Pillow byte for byte): the horizontal pass runs
first, the intermediate is bytes, a pass whose extent does not change is skipped; per pass

    scale = in / out;  fs = max(scale, 1);  support = 2 fs;  ksize = 2 ceil(support) + 1
    center = (xx + 0.5) scale;  xmin = max(trunc(center - support + 0.5), 0);  n = min(trunc(center + support + 0.5), in) - xmin
    w[x] = bicubic((x + xmin - center + 0.5) / fs), a = -0.5, normalised by their left-to-right sum, rounded to 22 fractional bits
    out[xx] = clamp((2^21 + sum_x in[xmin + x] k[x]) >> 22, 0, 255)

all coefficients in IEEE double on the host; the device only multiplies bytes by int32 coefficients.  The value written is
table[channel][byte], where the (3, 256) table is built once with torch's own fp32 byte / 255 - mean / std (and its bf16 twin by
.to(bfloat16)): bit exact by construction.

On a CPU device the same tables run in numpy (the same bits).  On a CUDA device there is no fallback: the kernel runs or
prepare() raises.

Out of scope, left with the caller: JPEG decoding, depth and pose, images_raw, the choice of views, other filters and modes."""
import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22        # = _ext BQ_VIEW_PRECISION_BITS
COLS, DESC = 5, 4          # = _ext.VIEW_COLS, _ext.VIEW_DESC
LDS_BYTES = 65536          # = _ext.VIEW_LDS_BYTES: a workgroup's LDS, of which
NORM_BYTES = 4096          # hold the normalisation table and the rest the horizontal pass of the input rows a tile needs
TILE_ROWS = 32             # output rows per workgroup where the LDS image allows (less where it does not)
MAX_EXTENT = 16384


def _bicubic(t):
    t, a = np.abs(t), -0.5
    inner = ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    outer = (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return np.where(t < 1.0, inner, np.where(t < 2.0, outer, 0.0))


def coefficients(in_size, out_size):
    """one pass's table -> (bounds (out, 2) int32 = xmin and n, k (out, ksize) int32, zero behind n).  in == out: the identity
    xmin = x, n = 1, k = 2^22, which gives the byte itself -- the skipped pass."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size), np.ones(out_size, dtype=np.int64)], 1).astype(np.int32)
        return bounds, np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = 2 * int(np.ceil(support)) + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0.0).astype(np.int64)
    n = np.minimum(np.trunc(center + support + 0.5), float(in_size)).astype(np.int64) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    w = _bicubic(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * (1.0 / fs))
    w = np.where(x < n[:, None], w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):                                   # left to right, as the definition sums
        ww = ww + w[:, j]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    one = float(1 << PRECISION_BITS)
    k = np.where(w >= 0, np.trunc(w * one + 0.5), np.trunc(w * one - 0.5)).astype(np.int32)
    return np.stack([xmin, n], 1).astype(np.int32), k


def norm_table(mean=CLIP_MEAN, std=CLIP_STD):
    """(3, 256) fp32: ToTensor and Normalize of every byte value, with torch's fp32 operations in their order"""
    mean, std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
    if len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
        raise ValueError("view_data: mean and std must hold three values, std none of them 0")
    b = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return b[None, :].sub(m[:, None]).div(s[:, None]).contiguous()


def _size(size):
    OH, OW = (size, size) if isinstance(size, int) else tuple(int(s) for s in size)
    if not (1 <= OH <= MAX_EXTENT and 1 <= OW <= MAX_EXTENT):
        raise ValueError("view_data: size %s outside [1, %d]" % ((OH, OW), MAX_EXTENT))
    return OH, OW


def _pick_tile(vbounds, OH, OW, target):
    """the tile height and the LDS rows it needs: the largest height <= target whose input rows (the vertical windows of a
    tile's rows, for every vertical table) fit the LDS image.  ValueError if not even one output row fits."""
    budget = (LDS_BYTES - NORM_BYTES) // (3 * OW)
    for th in range(max(1, min(int(target), OH)), 0, -1):
        starts = np.arange(0, OH, th)
        rows = max(int((np.maximum.reduceat(b[:, 0] + b[:, 1], starts) - np.minimum.reduceat(b[:, 0], starts)).max())
                   for b in vbounds)
        if rows <= budget:
            return th, max(rows, 1)
    raise ValueError("view_data: one output row of %d pixels needs %d input rows of the %d-wide intermediate, and %d fit the "
                     "%d bytes of LDS a workgroup holds (shrinking this far is not supported)"
                     % (OW, rows, OW, budget, LDS_BYTES - NORM_BYTES))


class _Plan(object):
    """the tables of a set of views for one output size: host arrays, and device tensors on a CUDA device"""

    def __init__(self, shapes, bases, OH, OW, device, tile_rows=None):
        self.OH, self.OW = OH, OW
        self.tables, slot, chunks, desc, off = {}, {}, [], [], 0
        views = np.zeros((len(shapes), COLS), dtype=np.int64)
        for i, ((H, W), base) in enumerate(zip(shapes, bases)):
            for col, key in ((3, (W, OW)), (4, (H, OH))):
                if key not in slot:
                    bounds, k = coefficients(*key)
                    slot[key] = len(desc)
                    self.tables[key] = (bounds, k)
                    desc.append((off, off + bounds.size, k.shape[1], key[0]))
                    chunks += [bounds.ravel(), k.ravel()]
                    off += bounds.size + k.size
                views[i, col] = slot[key]
            views[i, 0:3] = base, H, W
        self.views_host, self.slot = views, slot
        vbounds = [self.tables[k][0] for k in sorted(set((H, OH) for H, _ in shapes))]
        self.tile_rows, self.lds_rows = _pick_tile(vbounds, OH, OW, TILE_ROWS if tile_rows is None else tile_rows)
        if torch.device(device).type == "cuda":
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self.tab, self.desc = up(np.concatenate(chunks).astype(np.int32)), up(np.asarray(desc, dtype=np.int32))
            self.views = up(views)


def _pass_host(src, bounds, k):
    """src (in, M) bytes -> (out, M) bytes along the first axis"""
    idx = np.minimum(bounds[:, 0:1].astype(np.int64) + np.arange(k.shape[1])[None, :], src.shape[0] - 1)
    acc = np.full((bounds.shape[0], src.shape[1]), 1 << (PRECISION_BITS - 1), dtype=np.int64)
    wide = src.astype(np.int64)
    for x in range(k.shape[1]):                               # (k is zero behind a window's n)
        acc += wide[idx[:, x]] * k[:, x:x + 1].astype(np.int64)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _resize_host(img, htab, vtab):
    """(H, W, 3) bytes -> (OH, OW, 3) bytes: horizontal pass, bytes, vertical pass"""
    H, W = img.shape[:2]
    OW, OH = htab[0].shape[0], vtab[0].shape[0]
    mid = _pass_host(img.transpose(1, 0, 2).reshape(W, H * 3), *htab).reshape(OW, H, 3).transpose(1, 0, 2)
    return _pass_host(np.ascontiguousarray(mid).reshape(H, OW * 3), *vtab).reshape(OH, OW, 3)


def _unfold(x, p):
    """(N, 3, OH, OW) -> (N, (OH / p)(OW / p), 3 p p): the element order of vit.PatchEmbed.forward"""
    N, C, H, W = x.shape
    return x.reshape(N, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(N, (H // p) * (W // p), C * p * p)


class _Format(object):
    """output type and layout of a batch, with the normalisation table in that type on `device`"""

    def __init__(self, who, OH, OW, mean, std, dtype, layout, patch, device):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("%s: dtype must be torch.float32 or torch.bfloat16, got %s" % (who, dtype))
        if layout not in ("nchw", "patches"):
            raise ValueError("%s: layout must be 'nchw' or 'patches', got %r" % (who, layout))
        self.patch = int(patch) if layout == "patches" else 0
        if layout == "patches" and (self.patch < 1 or OH % self.patch or OW % self.patch):
            raise ValueError("%s: patch = %s does not divide the size %d x %d" % (who, patch, OH, OW))
        self.dtype, self.layout = dtype, layout
        self.norm = norm_table(mean, std)
        self.table = self.norm.to(dtype).to(device)
        p = self.patch
        self.item = ((OH // p) * (OW // p), 3 * p * p) if p else (3, OH, OW)

    def host(self, bytes_hwc):
        """(N, OH, OW, 3) bytes -> the batch on the host: the lookup, then pure data movement"""
        t = self.norm.to(self.dtype)
        x = torch.from_numpy(np.ascontiguousarray(bytes_hwc)).permute(0, 3, 1, 2).long()           # (N, 3, OH, OW)
        vals = torch.stack([t[c][x[:, c]] for c in range(3)], 1)
        return _unfold(vals, self.patch).contiguous() if self.patch else vals.contiguous()


def _as_frame(f, i):
    a = f.cpu().numpy() if torch.is_tensor(f) else np.asarray(f)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("ViewStore: frame %d must be an (H >= 1, W >= 1, 3) uint8 array, got %s %s" % (i, a.dtype, a.shape))
    if max(a.shape[:2]) > MAX_EXTENT:
        raise ValueError("ViewStore: frame %d is %d x %d; extents up to %d are supported" % (i, a.shape[0], a.shape[1], MAX_EXTENT))
    return np.ascontiguousarray(a)


class ViewStore(object):
    """RGB frames of any sizes packed once into one byte tensor on `device`: view i owns bytes base[i] .. base[i] + 3 H_i W_i
    (int64 offsets).  plan(OH, OW) builds, once per output size, the coefficient and bounds tables of every distinct input
    width and height in double on the host.  Raises ValueError for frames that are not (H, W, 3) uint8."""

    def __init__(self, frames, device):
        self.device = torch.device(device)
        frames = [_as_frame(f, i) for i, f in enumerate(frames)]
        if not frames:
            raise ValueError("ViewStore: no frames")
        self.shapes = [f.shape[:2] for f in frames]
        base = np.zeros(len(frames) + 1, dtype=np.int64)
        base[1:] = np.cumsum([f.size for f in frames], dtype=np.int64)
        self.base = base
        packed = np.empty(int(base[-1]), dtype=np.uint8)
        for f, lo in zip(frames, base[:-1]):
            packed[lo:lo + f.size] = f.ravel()
        self.pixels = torch.from_numpy(packed).to(self.device)
        self._plans = {}

    def __len__(self):
        return len(self.shapes)

    @property
    def nbytes(self):
        return self.pixels.numel()

    def plan(self, OH, OW, tile_rows=None):
        key = (OH, OW, tile_rows)
        if key not in self._plans:
            self._plans[key] = _Plan(self.shapes, self.base[:-1], OH, OW, self.device, tile_rows)
        return self._plans[key]

    def frame(self, i):
        """view i as an (H, W, 3) numpy array (a host copy)"""
        H, W = self.shapes[i]
        return self.pixels[int(self.base[i]):int(self.base[i + 1])].cpu().numpy().reshape(H, W, 3)


def _run_host(pixels, plan, fmt, index):
    """the definition in numpy for the views `index` (a flat list) of a packed byte array"""
    done, out = {}, []
    for v in index:
        if v not in done:
            base, H, W = (int(t) for t in plan.views_host[v, 0:3])
            img = pixels[base:base + 3 * H * W].reshape(H, W, 3)
            done[v] = _resize_host(img, plan.tables[(W, plan.OW)], plan.tables[(H, plan.OH)])
        out.append(done[v])
    return fmt.host(np.stack(out))


class ViewBatcher(object):
    """prepare() turns view indices into the image tensor of a batch under the reference's data-dict key: "images"
    (B, V, 3, OH, OW) in layout "nchw", or (B, V, (OH / p)(OW / p), 3 p p) in layout "patches" -- the rows vit.PatchEmbed's GEMM
    reads, so its unfold (and with dtype=torch.bfloat16 the cast) is not run.  size: an int or (OH, OW).

    On a CUDA store a batch is one launch (_ext.VIEW_CALLS); with an index tensor on the device the host waits for nothing and
    the call can be captured in a HIP graph; with `out` no tensor is allocated.  The tile height is chosen here from the
    store's vertical tables; ValueError if a single output row's input rows do not fit a workgroup's LDS."""

    def __init__(self, store, size=480, mean=CLIP_MEAN, std=CLIP_STD, dtype=torch.float32, layout="nchw", patch=16,
                 tile_rows=None):
        self.store = store
        self.OH, self.OW = _size(size)
        self.format = _Format("ViewBatcher", self.OH, self.OW, mean, std, dtype, layout, patch, store.device)
        self.plan = store.plan(self.OH, self.OW, tile_rows)
        self.tile_rows, self.lds_rows = self.plan.tile_rows, self.plan.lds_rows
        self._index = {}            # (B, V) -> device buffer for indices that arrive from the host

    def spec(self, B, V=1):
        """key -> (shape, dtype) of a batch"""
        return {"images": ((B, V) + self.format.item, self.format.dtype)}

    def empty(self, B, V=1):
        return {k: torch.empty(shape, dtype=dtype, device=self.store.device) for k, (shape, dtype) in self.spec(B, V).items()}

    def prepare(self, view_index, out=None):
        """view_index: (B,) or (B, V) indices into the store -- a sequence, an array, or an integer tensor; a tensor on the
        store's CUDA device is read by the kernel as it is (not checked on the host: the kernel clamps it into range), anything
        else is checked here (ValueError) and uploaded.  (B,) gives V = 1.  out: a dict; its "images" tensor is written in place
        (a shape, dtype, device or layout mismatch raises ValueError), a missing one is allocated and added; other keys are left
        alone.  Returns out."""
        store, dev = self.store, self.store.device
        on_device = torch.is_tensor(view_index) and view_index.device == dev and dev.type == "cuda"
        if on_device:
            idx = view_index
            if idx.dtype not in (torch.int64, torch.int32):
                raise ValueError("ViewBatcher.prepare: view_index must be an int64 or int32 tensor, got %s" % idx.dtype)
        else:
            host = view_index.cpu().numpy() if torch.is_tensor(view_index) else np.asarray(view_index)
            if host.dtype.kind not in "iu":
                raise ValueError("ViewBatcher.prepare: view_index must hold integers, got %s" % host.dtype)
            idx = host.astype(np.int64)
        if idx.ndim not in (1, 2) or idx.shape[0] < 1 or idx.shape[-1] < 1:
            raise ValueError("ViewBatcher.prepare: view_index must be (B,) or (B, V), got %s" % (tuple(idx.shape),))
        B, V = idx.shape[0], (idx.shape[1] if idx.ndim == 2 else 1)
        if not on_device and (idx.min() < 0 or idx.max() >= len(store)):
            raise ValueError("ViewBatcher.prepare: view index outside [0, %d)" % len(store))
        (shape, dtype), = self.spec(B, V).values()
        out = {} if out is None else out
        if "images" in out:
            t = out["images"]
            if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
                raise ValueError("ViewBatcher.prepare: out['images'] must be %s %s, got %s" % (
                    dtype, tuple(shape), "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
            if t.device != dev or not t.is_contiguous():
                raise ValueError("ViewBatcher.prepare: out['images'] must be a contiguous tensor on %s" % dev)
        else:
            out["images"] = torch.empty(shape, dtype=dtype, device=dev)
        images = out["images"]
        if dev.type == "cuda":
            from . import _ext
            with torch.cuda.device(dev):
                if on_device:
                    flat = idx.reshape(-1).to(torch.int64)
                    flat = flat if flat.is_contiguous() else flat.contiguous()
                else:
                    if (B, V) not in self._index:
                        self._index[(B, V)] = torch.empty(B * V, dtype=torch.int64, device=dev)
                    flat = self._index[(B, V)]
                    flat.copy_(torch.from_numpy(idx.reshape(-1)).pin_memory(), non_blocking=True)
                _ext.view_prep(store.pixels, self.plan.views, self.plan.tab, self.plan.desc, flat, self.format.table,
                               images.view((B * V,) + self.format.item), self.OH, self.OW, self.tile_rows, self.lds_rows,
                               patch=self.format.patch)
        else:
            got = _run_host(store.pixels.numpy(), self.plan, self.format, [int(v) for v in idx.reshape(-1)])
            images.copy_(got.view(images.shape))
        return out


_PLANS = {}     # (N, H, W, OH, OW, device) -> _Plan of preprocess_views, the latest few
_FORMATS = {}


def preprocess_views(frames_u8, size, mean=CLIP_MEAN, std=CLIP_STD, dtype=torch.float32, layout="nchw", patch=16):
    """(N, H, W, 3) uint8 frames of one size, on any device -> (N, 3, OH, OW), or (N, (OH / p)(OW / p), 3 p p) for layout
    "patches", on the frames' device: ViewBatcher's output without a store (blip_itm.encode_views runs it per chunk)."""
    if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 \
            or min(frames_u8.shape) < 1:
        raise ValueError("preprocess_views: frames must be an (N >= 1, H, W, 3) uint8 tensor, got %s"
                         % ("%s %s" % (frames_u8.dtype, tuple(frames_u8.shape)) if torch.is_tensor(frames_u8) else type(frames_u8)))
    N, H, W = frames_u8.shape[:3]
    if max(H, W) > MAX_EXTENT:
        raise ValueError("preprocess_views: frames are %d x %d; extents up to %d are supported" % (H, W, MAX_EXTENT))
    OH, OW = _size(size)
    dev = frames_u8.device
    key = (N, H, W, OH, OW, str(dev))
    if key not in _PLANS:
        while len(_PLANS) >= 8:
            _PLANS.pop(next(iter(_PLANS)))
        _PLANS[key] = _Plan([(H, W)] * N, np.arange(N, dtype=np.int64) * (3 * H * W), OH, OW, dev)
    plan = _PLANS[key]
    fkey = (OH, OW, tuple(mean), tuple(std), dtype, layout, int(patch), str(dev))
    if fkey not in _FORMATS:
        while len(_FORMATS) >= 8:
            _FORMATS.pop(next(iter(_FORMATS)))
        _FORMATS[fkey] = _Format("preprocess_views", OH, OW, mean, std, dtype, layout, patch, dev)
    fmt = _FORMATS[fkey]
    pixels = frames_u8.contiguous().view(-1)
    if dev.type != "cuda":
        return _run_host(pixels.numpy(), plan, fmt, range(N))
    from . import _ext
    with torch.cuda.device(dev):
        if not hasattr(plan, "index"):
            plan.index = torch.arange(N, dtype=torch.int64, device=dev)
        out = torch.empty((N,) + fmt.item, dtype=dtype, device=dev)
        return _ext.view_prep(pixels, plan.views, plan.tab, plan.desc, plan.index, fmt.table, out, OH, OW, plan.tile_rows,
                              plan.lds_rows, patch=fmt.patch)
