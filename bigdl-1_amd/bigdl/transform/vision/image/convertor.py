"""Decoding and batching (``DL/transform/vision/image/{Convertor,MTImageFeatureToBatch}.scala``).

* ``BytesToMat`` decodes encoded bytes (JPEG/PNG/…; PIL stands in for OpenCV ``imdecode``) into
  a BGR float ``[H, W, C]`` mat; ``PixelBytesToMat`` reinterprets raw HWC uint8 pixels.
* ``MatToTensor`` / ``MatToFloats`` / ``ImageFrameToSample`` / ``ImageFeatureToMiniBatch``.
* ``MTImageFeatureToBatch``: the training-batch assembler.  On a GPU it uploads the uint8 pixels
  once (pinned, async) and runs the fused crop + mirror + per-channel normalise + bf16 NHWC cast
  HIP kernel (``ops.image_crop_flip_norm``, kernel K25) — the device-side replacement of the
  reference's per-image OpenCV loop.  With ``device_augment=True`` the tail of the transformer chain
  (``RandomAlterAspect``, crop, mirror, normalise) is lowered too: the decoder's uint8 pixels go up in
  one packed buffer and ``ops.image_resample_norm`` (kernel K25b) resizes on the device.
"""
from __future__ import annotations

import io
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from ....dataset import MiniBatch, Sample, SampleToMiniBatch
from ....utils.engine import Engine
from ....utils.random import RNG
from ....utils.table import Table
from .image_feature import FeatureTransformer, ImageFeature


def decode_bytes(b: bytes) -> torch.Tensor:
    from PIL import Image
    img = Image.open(io.BytesIO(b))
    if img.mode not in ("RGB", "L"):
        img = img.convert("RGB")
    a = np.asarray(img, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    else:
        a = a[:, :, ::-1]  # RGB → BGR
    return torch.from_numpy(np.ascontiguousarray(a))


MAT_U8 = "matU8"


def _set_decoded(f: ImageFeature, u8: torch.Tensor):
    """The float mat every transformer works on, plus the decoder's uint8 pixels next to it (with the mat
    they belong to and its version, so a later ``set_mat`` or in-place edit disowns them): the device
    augmentation uploads those 1-byte pixels instead of the floats."""
    f.set_mat(u8.float())
    m = f.opencv_mat()
    f[MAT_U8] = (u8, m, m._version)


def decoded_u8(f: ImageFeature) -> Optional[torch.Tensor]:
    """The uint8 pixels of ``f``'s mat when it is still exactly what the decoder produced, else None."""
    rec = f.get(MAT_U8)
    if rec is None:
        return None
    u8, m, ver = rec
    cur = f.get(ImageFeature.mat)
    return u8 if (cur is m and m._version == ver) else None


class BytesToMat(FeatureTransformer):
    def __init__(self, byte_key: str = ImageFeature.bytes):
        self.key = byte_key

    def transform_mat(self, f):
        _set_decoded(f, decode_bytes(f[self.key]))


class PixelBytesToMat(FeatureTransformer):
    """Raw pixel bytes in HWC order; the size comes from ``originalSize``."""

    def __init__(self, byte_key: str = ImageFeature.bytes):
        self.key = byte_key

    def transform_mat(self, f):
        h, w, c = f[ImageFeature.originalSize]
        a = np.frombuffer(f[self.key], dtype=np.uint8).reshape(h, w, c)
        _set_decoded(f, torch.from_numpy(a.copy()))


class MatToFloats(FeatureTransformer):
    def __init__(self, valid_height: int = 300, valid_width: int = 300, valid_channels: int = 3,
                 out_key: str = ImageFeature.floats, share_buffer: bool = True):
        self.h, self.w, self.c, self.key = valid_height, valid_width, valid_channels, out_key

    def transform_mat(self, f):
        m = f.opencv_mat() if ImageFeature.mat in f else torch.zeros(self.h, self.w, self.c)
        f[self.key] = m.reshape(-1).float()


class MatToTensor(FeatureTransformer):
    """HWC BGR mat → CHW tensor (RGB with ``to_rgb``) under ``tensor_key``."""

    def __init__(self, to_rgb: bool = False, tensor_key: str = ImageFeature.imageTensor, share_buffer: bool = True,
                 greyToRGB: bool = False):
        self.to_rgb, self.key, self.grey_to_rgb = to_rgb, tensor_key, greyToRGB

    def transform_mat(self, f):
        t = f.to_chw(self.to_rgb)
        if self.grey_to_rgb and t.shape[0] == 1:
            t = t.expand(3, -1, -1).contiguous()
        f[self.key] = t


class ImageFrameToSample(FeatureTransformer):
    def __init__(self, input_keys: Sequence[str] = (ImageFeature.imageTensor,), target_keys: Sequence[str] = None,
                 sample_key: str = ImageFeature.sample):
        self.inputs, self.targets, self.key = list(input_keys), list(target_keys or []), sample_key

    def transform_mat(self, f):
        feats = [f[k] for k in self.inputs]
        labs = [torch.as_tensor(f[k], dtype=torch.float32).reshape(-1) for k in self.targets if k in f]
        f[self.key] = Sample(feats, labs if labs else None)


class ImageFeatureToMiniBatch:
    """ImageFeatures (with ``sample``) → MiniBatches of ``batch_size``."""

    def __init__(self, batch_size: int, feature_padding=None, label_padding=None, partition_num=None,
                 sample_key: str = ImageFeature.sample):
        self.stm = SampleToMiniBatch(batch_size, feature_padding, label_padding, partition_num)
        self.key = sample_key

    def __call__(self, features):
        return self.stm(f[self.key] for f in features if f.is_valid())

    apply = __call__


def flatten_transformers(t) -> List[FeatureTransformer]:
    """``a >> b >> Pipeline([c, d])`` → ``[a, b, c, d]``."""
    from .image_feature import ChainedFeatureTransformer, Pipeline
    if t is None:
        return []
    if type(t) is ChainedFeatureTransformer:
        return flatten_transformers(t.first) + flatten_transformers(t.last)
    if type(t) is Pipeline:
        return [u for s in t.transformers for u in flatten_transformers(s)]
    return [t]


class LoweredTail:
    """The tail of a transformer chain that one ``ops.image_resample_norm`` launch replaces.

    Recognised, in this order and each optional: ``RandomAlterAspect``; ``RandomCropper`` | ``CenterCrop`` |
    ``RandomCrop``; ``HFlip`` (or the cropper's mirror); ``ChannelNormalize`` | ``ChannelScaledNormalizer``;
    ``MatToTensor``.  ``prefix`` is what stays on the host.  Anything else from the first lowered
    transformer on is a ``ValueError`` naming it: nothing is dropped silently."""

    def __init__(self, transformer):
        from . import augmentation as A
        stages = {A.RandomAlterAspect: 0, A.RandomCropper: 1, A.CenterCrop: 1, A.RandomCrop: 1, A.HFlip: 2,
                  A.ChannelNormalize: 3, A.ChannelScaledNormalizer: 3, MatToTensor: 4}
        flat = flatten_transformers(transformer)
        first = next((i for i, t in enumerate(flat) if type(t) in stages), len(flat))
        self.prefix, tail = flat[:first], flat[first:]
        self.alter = self.cropper = self.norm = None
        self.hflip = False
        last = -1
        for t in tail:
            st = stages.get(type(t))
            if st is None or st <= last:
                raise ValueError(f"device_augment cannot lower {type(t).__name__} at this place of the chain "
                                 "(order: RandomAlterAspect, crop, HFlip, normalise, MatToTensor)")
            last = st
            if st == 0:
                self.alter = t
            elif st == 1:
                self.cropper = t
            elif st == 2:
                self.hflip = True
            elif st == 3:
                self.norm = t
        if self.alter is not None:
            if self.alter.mode not in ("LINEAR", "CUBIC"):
                raise ValueError(f"device_augment resamples LINEAR or CUBIC, not {self.alter.mode!r}")
            c = self.cropper
            if c is not None and (c.cw, c.ch) != (self.alter.L, self.alter.L):
                raise ValueError(f"a {c.cw}×{c.ch} {type(c).__name__} after RandomAlterAspect(crop_length="
                                 f"{self.alter.L}) does not compose into one source rectangle")
        self.interp = self.alter.mode if self.alter is not None else "LINEAR"

    def draw(self, h: int, w: int, channels: int):
        """The draws the host transformers would make for one ``h × w`` image, in their order →
        the source rectangle ``(y, x, ch, cw)``, the size it is resized to, and the mirror flag."""
        from . import augmentation as A
        y = x = 0
        ch, cw = h, w
        oh = ow = None  # None: not resized
        flip = False
        if self.alter is not None:
            y, x, ch, cw = self.alter.draw(h, w)
            oh = ow = self.alter.L
        c = self.cropper
        if c is not None:
            ih, iw = (oh, ow) if oh is not None else (ch, cw)
            if type(c) is A.RandomCropper:
                if c.channels < channels:
                    raise ValueError("device_augment does not lower a RandomCropper that drops channels")
                cy, cx, flip = c.draw(ih, iw)
                wy, wx, wh, ww = cy, cx, min(c.ch, ih - cy), min(c.cw, iw - cx)
            else:
                wy, wx, wh, ww = A.Crop.window(ih, iw, *c.box_for(ih, iw), c.normalized, c.is_clip)
                wh, ww = min(wh, ih - wy), min(ww, iw - wx)
            if oh is None:
                if wy < 0 or wx < 0 or wh <= 0 or ww <= 0:
                    raise ValueError(f"{type(c).__name__} window outside the {ih}×{iw} image")
                y, x, ch, cw = y + wy, x + wx, wh, ww
            elif (wy, wx, wh, ww) != (0, 0, oh, ow):  # the constructor admitted only the identity crop
                raise ValueError("crop after RandomAlterAspect is not the identity")
        return (y, x, ch, cw), (oh, ow), bool(flip) != self.hflip

    def norm_params(self, channels: int):
        """(mean, std) of the lowered normaliser, in mat (BGR) channel order."""
        from . import augmentation as A
        n = self.norm
        if n is None:
            return [0.0] * channels, [1.0] * channels
        if type(n) is A.ChannelScaledNormalizer:
            if channels != len(n.means):
                raise ValueError("ChannelScaledNormalizer needs a 3-channel mat")
            return [float(v) for v in n.means], [1.0 / n.scale] * channels
        return [float(v) for v in n.means[:channels]], [float(v) for v in n.stds[:channels]]


class MTImageFeatureToBatch:
    """Classification batches of ``width × height``: each feature is transformed by
    ``transformer`` on ``num_threads`` host threads (decode, resize, jitter …); the final crop /
    mirror / normalise / cast runs either per image on the host, or — ``device="cuda"`` — as one
    fused HIP kernel over the whole batch.  Output: MiniBatch(input NCHW-logical channels-last,
    target 1-based labels).

    ``device_augment=True`` also takes the tail of ``transformer`` (:class:`LoweredTail`: random-area /
    random-aspect crop, resize, crop, mirror, normalise) off the host: the host threads run only what
    precedes it, the parameters are drawn from the framework ``RNG`` on the calling thread in feature
    order — the draws the host transformers would make — and one ``ops.image_resample_norm`` launch
    (the reference operator on a CPU device) writes the batch from one packed upload of the mats
    (uint8 when they are still the decoder's pixels, else fp32)."""

    def __init__(self, width: int, height: int, batch_size: int, transformer: Optional[FeatureTransformer] = None,
                 to_rgb: bool = True, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), random_crop: bool = False,
                 mirror: bool = False, device: Optional[str] = None, num_threads: int = 4,
                 out_dtype: Optional[torch.dtype] = None, device_augment: bool = False):
        self.w, self.h, self.bs = width, height, batch_size
        self.transformer = transformer
        self.to_rgb, self.mean, self.std = to_rgb, list(mean), list(std)
        self.random_crop, self.mirror = random_crop, mirror
        self.device = torch.device(device) if device else Engine.device()
        self.pool = ThreadPoolExecutor(max(1, num_threads))
        self.out_dtype = out_dtype
        self.lowered = LoweredTail(transformer) if device_augment else None
        if self.lowered is not None and self.lowered.alter is not None and \
                (self.lowered.alter.L, self.lowered.alter.L) != (height, width):
            raise ValueError(f"RandomAlterAspect(crop_length={self.lowered.alter.L}) does not give the "
                             f"{width}×{height} batch: the batch's own crop would not compose")

    def _prep(self, f: ImageFeature):
        if self.lowered is not None:
            for t in self.lowered.prefix:
                f = t.transform(f)
        elif self.transformer is not None:
            f = self.transformer.transform(f)
        return f

    def __call__(self, features):
        buf = []
        for f in features:
            buf.append(f)
            if len(buf) == self.bs:
                yield self._make(buf)
                buf = []
        if buf:
            yield self._make(buf)

    apply = __call__

    def _make_lowered(self, feats: List[ImageFeature]) -> MiniBatch:
        low = self.lowered
        mats = [f.opencv_mat() for f in feats]
        C = mats[0].shape[2]
        if any(m.shape[2] != C for m in mats):
            raise ValueError("device_augment needs one channel count per batch")
        rects, flips = [], []
        for m in mats:  # calling thread, feature order: the host transformers' draws, then the batch's own
            (y, x, ch, cw), (oh, _), fl = low.draw(m.shape[0], m.shape[1], C)
            if oh is None:
                if ch < self.h or cw < self.w:
                    raise ValueError(f"a {cw}×{ch} image cannot give a {self.w}×{self.h} batch crop")
                if self.random_crop:
                    oy = int(RNG.uniform(0, ch - self.h + 1)) if ch > self.h else 0
                    ox = int(RNG.uniform(0, cw - self.w + 1)) if cw > self.w else 0
                else:
                    oy, ox = (ch - self.h) // 2, (cw - self.w) // 2
                # the batch's crop is taken from the chain's (already mirrored) image
                y, x = y + oy, x + (cw - self.w - ox if fl else ox)
                ch, cw = self.h, self.w
            if self.mirror and RNG.uniform(0, 1) < 0.5:
                fl = not fl
            rects.append([y, x, ch, cw])
            flips.append(int(fl))
        # one packed upload: the decoder's uint8 pixels when every mat still is what it decoded, else fp32
        u8 = [decoded_u8(f) for f in feats]
        pix = u8 if all(u is not None for u in u8) else [m.float() for m in mats]
        pin = self.device.type == "cuda"
        packed = torch.empty(sum(p.numel() for p in pix), dtype=pix[0].dtype, pin_memory=pin)
        at = 0
        for p in pix:
            packed[at:at + p.numel()].copy_(p.reshape(-1))
            at += p.numel()
        m1, s1 = low.norm_params(C)
        if self.to_rgb and C == 3:
            m1, s1 = m1[::-1], s1[::-1]
        m2 = (self.mean[::-1] if not self.to_rgb else self.mean)[:C]
        s2 = (self.std[::-1] if not self.to_rgb else self.std)[:C]
        m2, s2 = list(m2) + [0.0] * (C - len(m2)), list(s2) + [1.0] * (C - len(s2))
        # ((v − m1)/s1 − m2)/s2 = (v − (m1 + m2·s1)) / (s1·s2), in output channel order
        mean = [a + b * s for a, b, s in zip(m1, m2, s1)]
        std = [a * b for a, b in zip(s1, s2)]
        from .... import ops
        x = ops.image_resample_norm(packed.to(self.device, non_blocking=True), torch.tensor(rects),
                                    torch.tensor(flips, dtype=torch.int32), self.h, self.w, mean, std, self.to_rgb,
                                    low.interp, self.out_dtype or (Engine.compute_dtype() if pin else torch.float32),
                                    sizes=torch.tensor([[m.shape[0], m.shape[1], C] for m in mats]))
        labels = torch.tensor([float(f.get_label() if f.get_label() is not None else 0) for f in feats])
        return MiniBatch(x, labels.to(self.device))

    def _make(self, feats: List[ImageFeature]) -> MiniBatch:
        feats = [f for f in self.pool.map(self._prep, feats) if f.is_valid()]
        if self.lowered is not None:
            return self._make_lowered(feats)
        mats = [f.opencv_mat() for f in feats]
        H = min(m.shape[0] for m in mats)
        W = min(m.shape[1] for m in mats)
        C = mats[0].shape[2]
        B = len(mats)
        oy, ox, fl = [], [], []
        for m in mats:
            hh, ww = m.shape[0], m.shape[1]
            if self.random_crop:
                oy.append(int(RNG.uniform(0, hh - self.h + 1)) if hh > self.h else 0)
                ox.append(int(RNG.uniform(0, ww - self.w + 1)) if ww > self.w else 0)
            else:
                oy.append(max(0, (hh - self.h) // 2))
                ox.append(max(0, (ww - self.w) // 2))
            fl.append(1 if (self.mirror and RNG.uniform(0, 1) < 0.5) else 0)
        labels = torch.tensor([float(f.get_label() if f.get_label() is not None else 0) for f in feats])
        # gather the crop windows (plus a margin-free stack) so the kernel sees one dense batch
        crops = torch.stack([m[y:y + self.h, x:x + self.w] for m, y, x in zip(mats, oy, ox)])
        from .... import ops
        mean = self.mean[::-1] if not self.to_rgb else self.mean
        std = self.std[::-1] if not self.to_rgb else self.std
        x = ops.image_crop_flip_norm(crops.to(self.device, non_blocking=True), torch.zeros(B, dtype=torch.int32),
                                     torch.zeros(B, dtype=torch.int32), torch.tensor(fl, dtype=torch.int32),
                                     self.h, self.w, mean, std, self.to_rgb,
                                     self.out_dtype or (Engine.compute_dtype() if self.device.type == "cuda"
                                                        else torch.float32))
        return MiniBatch(x, labels.to(self.device))
