"""Device-side augmentation, host half: the fp64 oracle of the crop → resample → mirror → normalise rule,
the fp32 torch operator (``ops.reference.image_resample_norm``) against it, the lowering of a transformer
chain's tail in ``MTImageFeatureToBatch(device_augment=True)``, the raw mode of the native batch loader
and the training CLI flags.  ``tests/test_image_augment.py`` imports the oracle and the case set from here.

The oracle is a transcription of the rule, not of any implementation: per axis
``num = (2o+1)·n_in − n_out``, ``den = 2·n_out``, ``f = ⌊num/den⌋``, ``t = (num mod den)/den``; taps
``f−1…f+2`` (CUBIC, A = −0.75) or ``f, f+1`` (LINEAR) clamped to the rectangle; CUBIC clamped to
[0, 255]; mirror; ``(v − mean)·(1/std)``.
"""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from bigdl.ops import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------- fp64 oracle
A = -0.75


def taps64(n_in, n_out, interp):
    """[n_out, n_in] fp64 filter matrix of one axis (weights of clamped taps accumulate)."""
    m = np.zeros((n_out, n_in), dtype=np.float64)
    den = 2 * n_out
    for o in range(n_out):
        num = (2 * o + 1) * n_in - n_out
        f = num // den
        t = (num - f * den) / den
        if interp == "CUBIC":
            u, s = t + 1.0, 1.0 - t
            w0 = ((A * u - 5 * A) * u + 8 * A) * u - 4 * A
            w1 = ((A + 2) * t - (A + 3)) * t * t + 1
            w2 = ((A + 2) * s - (A + 3)) * s * s + 1
            taps = [(f - 1, w0), (f, w1), (f + 1, w2), (f + 2, 1.0 - w0 - w1 - w2)]
        else:
            taps = [(f, 1.0 - t), (f + 1, t)]
        for i, w in taps:
            m[o, min(max(i, 0), n_in - 1)] += w
    return m


def oracle(images, rows, out_h, out_w, mean, std, to_rgb, interp):
    """``images``: list of [H, W, C] arrays; ``rows``: (image, y0, x0, ch, cw, flip) → [B, OH, OW, C] fp64."""
    outs = []
    for k, y0, x0, ch, cw, fl in rows:
        r = images[k][y0:y0 + ch, x0:x0 + cw].astype(np.float64)
        v = np.einsum("oy,yxc,px->opc", taps64(ch, out_h, interp), r, taps64(cw, out_w, interp))
        if interp == "CUBIC":
            v = np.clip(v, 0.0, 255.0)
        if fl:
            v = v[:, ::-1]
        C = v.shape[2]
        if to_rgb and C == 3:
            v = v[:, :, ::-1]
        outs.append((v - np.asarray(mean[:C], np.float64)) * (1.0 / np.asarray(std[:C], np.float64)))
    return np.stack(outs)


# ------------------------------------------------------------------------------------------- case set
SIZES = [(29, 37), (50, 40), (12, 9), (16, 16), (2, 3)]  # (H, W): 37×29, 40×50, 9×12, 16×16, 3×2 (W×H)
MEAN = (104.0, 117.0, 123.0, 110.0)
STD = (58.4, 57.1, 57.4, 60.0)
# 16×16 and 20×24 (OH ≠ OW); 10×12 is there for the 3.4× downsample, which no image of the batch is large
# enough for at the other two sizes (50 rows → 16 is 3.125×)
OUT_SIZES = [(16, 16), (20, 24), (10, 12)]


def rect_rows(out_h, out_w):
    """(image, y0, x0, ch, cw) — every rectangle kind of the set, for each image it fits."""
    rows = []
    for k, (H, W) in enumerate(SIZES):
        rows.append((k, 0, 0, H, W))  # the whole image
        if H >= 6 and W >= 6:
            rows += [(k, 0, 1, H // 2, W - 2), (k, H - H // 2, 1, H // 2, W - 2),  # top, bottom border
                     (k, 1, 0, H - 2, W // 2), (k, 1, W - W // 2, H - 2, W // 2),  # left, right border
                     (k, 2, 3, H - 3, 1), (k, 1, W - 2, H - 2, 2)]  # width 1 and 2: every x tap clamps
        if H >= 3 and W >= 3:
            rows.append((k, H - 2, W - 2, 2, 2))  # 2×2 → 8× upsample at 16×16
        else:
            rows.append((k, 0, 0, 2, 2))
        if H >= out_h and W >= out_w:
            rows.append((k, H - out_h, (W - out_w) // 2, out_h, out_w))  # the identity
        if H >= 34 and W >= 40:
            rows.append((k, 7, 0, 34, 40))  # 3.4× down at OH = 10; 2.1× / 1.7× at the other sizes
            rows.append((k, 0, 0, 50, 40))  # 3.125× down at OH = 16: taps skip source pixels
    rows.append((0, 3, 5, 21, 13))  # odd x0, odd W·C pitch (37·3 = 111 B rows)
    rows.append((0, 4, 7, 9, 28))
    return rows


@functools.lru_cache(maxsize=None)
def case(C, out_hw, src_float, seed=0):
    """The packed batch: (images, packed 1-D torch buffer, sizes [B, 3], offsets [B], rects [B, 4], flip [B],
    oracle rows).  One descriptor row per rectangle; rows share the five images."""
    rng = np.random.default_rng(seed + 17 * C + (1000 if src_float else 0))
    images = []
    for H, W in SIZES:
        if src_float:
            images.append((rng.random((H, W, C)) * 255.0).astype(np.float32))
        else:
            images.append(rng.integers(0, 256, size=(H, W, C), dtype=np.uint8))
    item = 4 if src_float else 1
    starts = np.concatenate([[0], np.cumsum([im.size * item for im in images])])[:-1]
    packed = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images]))
    rr = rect_rows(*out_hw)
    flip = [(i * 7 + 3) % 3 == 0 for i in range(len(rr))]  # mixed within the batch
    sizes = torch.tensor([[SIZES[k][0], SIZES[k][1], C] for k, *_ in rr])
    offsets = torch.tensor([int(starts[k]) for k, *_ in rr])
    rects = torch.tensor([list(r[1:]) for r in rr])
    rows = [r + (int(f),) for r, f in zip(rr, flip)]
    return images, packed, sizes, offsets, rects, torch.tensor(flip, dtype=torch.int32), rows


@functools.lru_cache(maxsize=None)
def expected(C, out_hw, src_float, interp, to_rgb):
    """(fp64 oracle [B, C, OH, OW], E_torch) of a case: the oracle once, shared by every test that needs it."""
    images, packed, sizes, offsets, rects, flip, rows = case(C, out_hw, src_float)
    want = oracle(images, rows, out_hw[0], out_hw[1], MEAN, STD, to_rgb, interp).transpose(0, 3, 1, 2)
    got = R.image_resample_norm(packed, rects, flip, out_hw[0], out_hw[1], MEAN, STD, to_rgb, interp,
                                torch.float32, sizes=sizes, offsets=offsets)
    e_torch = float(np.abs(got.double().numpy() - want).max())
    return want, e_torch


# ------------------------------------------------------------------------------------------- 1, 2: operator
@pytest.mark.parametrize("interp", ["LINEAR", "CUBIC"])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_reference_operator_against_fp64(C, interp):
    """The fp32 torch operator is within fp32 resampling error of the oracle (this error is E_torch, the
    yardstick of the kernel's bound).  Bound: torch forms the coordinate as a float product, which the
    issue measured at up to 0.007 grey levels at 224; at ≤ 50 pixels, /57 after normalising, 1e-3 is ample
    and anything structural (a wrong tap, clamp, mirror or channel) is O(1)."""
    for out_hw in OUT_SIZES:
        for src_float in (False, True):
            for to_rgb in (False, True):
                want, e = expected(C, out_hw, src_float, interp, to_rgb)
                print(f"image_aug_error reference C={C} out={out_hw} src={'f32' if src_float else 'u8'} "
                      f"{interp} to_rgb={int(to_rgb)} torch_fp32={e:.3e}")
                assert want.shape[1:] == (C,) + out_hw and e < 1e-3


@pytest.mark.parametrize("interp", ["LINEAR", "CUBIC"])
def test_identity_rectangle_is_crop_flip_norm(interp):
    rng = np.random.default_rng(3)
    src = torch.from_numpy(rng.integers(0, 256, size=(4, 20, 23, 3), dtype=np.uint8))
    oy, ox, fl = [0, 3, 8, 5], [7, 0, 2, 6], [0, 1, 1, 0]
    rects = torch.tensor([[y, x, 12, 16] for y, x in zip(oy, ox)])
    for flip in (fl, [0, 0, 0, 0]):
        for to_rgb in (False, True):
            a = R.image_resample_norm(src, rects, flip, 12, 16, (1, 2, 3), (2, 3, 4), to_rgb, interp)
            b = R.image_crop_flip_norm(src, oy, ox, flip, 12, 16, (1, 2, 3), (2, 3, 4), to_rgb)
            assert torch.equal(a, b)


def test_operator_rejects_bad_rectangles():
    src = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for rects in ([[0, 0, 9, 4], [0, 0, 4, 4]], [[0, 0, 0, 4], [0, 0, 4, 4]], [[-1, 0, 4, 4], [0, 0, 4, 4]],
                  [[0, 5, 4, 4], [0, 0, 4, 4]]):
        with pytest.raises(ValueError):
            R.image_resample_norm(src, torch.tensor(rects), [0, 0], 4, 4, (0, 0, 0), (1, 1, 1), False)
    with pytest.raises(ValueError):  # the second image would end past the buffer
        R.image_resample_norm(torch.zeros(100, dtype=torch.uint8), torch.tensor([[0, 0, 2, 2]] * 2), [0, 0], 4, 4,
                              (0,) * 3, (1,) * 3, False, sizes=torch.tensor([[4, 4, 3]] * 2),
                              offsets=torch.tensor([0, 60]))


# ------------------------------------------------------------------------------------------- 3, 4: lowering
def _features(n=8, seed=2):
    from bigdl.transform.vision.image import ImageFeature
    from bigdl.transform.vision.image.convertor import PixelBytesToMat
    rng = np.random.default_rng(seed)
    feats = []
    for i in range(n):
        h, w = int(rng.integers(20, 41)), int(rng.integers(20, 41))
        px = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        f = ImageFeature(px.tobytes(), label=float(i + 1))
        f[ImageFeature.originalSize] = (h, w, 3)
        feats.append(PixelBytesToMat().transform(f))
    return feats


def _chain(**alter):
    from bigdl.transform.vision.image import augmentation as A
    return (A.RandomAlterAspect(interp_mode="LINEAR", crop_length=16, **alter) >>
            A.RandomCropper(16, 16, True, "Random") >> A.ChannelScaledNormalizer(104, 117, 123, 0.0078125))


@pytest.mark.parametrize("alter", [{}, {"min_area_ratio": 4, "max_area_ratio": 4}],
                         ids=["drawn", "ten-failures"])
def test_lowered_draws_match_host_chain(alter):
    """Same seed, same draws in the same order: every image of the lowered batch is the host chain's image
    (both are fp32 torch bilinear of the same rectangle; a different draw would differ by O(1))."""
    from bigdl.transform.vision.image.convertor import MTImageFeatureToBatch
    from bigdl.utils.random import RNG
    for seed in (5, 6, 7):
        RNG.setSeed(seed)
        chain = _chain(**alter)
        host = [chain.transform(f.clone()).opencv_mat() for f in _features()]
        RNG.setSeed(seed)
        mt = MTImageFeatureToBatch(16, 16, 8, transformer=_chain(**alter), device="cpu", device_augment=True,
                                   to_rgb=False)
        batches = list(mt(_features()))
        assert len(batches) == 1
        x = batches[0].getInput()
        assert x.shape == (8, 3, 16, 16) and batches[0].getTarget().tolist() == [float(i + 1) for i in range(8)]
        for i in range(8):
            assert float((x[i] - host[i].permute(2, 0, 1)).abs().max()) <= 1e-4, (seed, i)
    if alter:  # ten failed attempts: the whole image, mirrored or not
        f = _features()[0]
        whole = torch.nn.functional.interpolate(f.opencv_mat().permute(2, 0, 1)[None], size=(16, 16),
                                                mode="bilinear", align_corners=False)[0]
        whole = (whole - torch.tensor([123.0, 117.0, 104.0])[:, None, None]) * 0.0078125
        assert min(float((host[0].permute(2, 0, 1) - w).abs().max()) for w in (whole, whole.flip(2))) <= 1e-4


def test_lowering_uploads_decoder_bytes_until_the_mat_changes():
    from bigdl.transform.vision.image import augmentation as A
    from bigdl.transform.vision.image.convertor import decoded_u8
    f = _features(1)[0]
    assert decoded_u8(f).dtype == torch.uint8 and torch.equal(decoded_u8(f).float(), f.opencv_mat())
    assert decoded_u8(f.clone()) is None  # a clone owns a new mat
    g = _features(1)[0]
    g.opencv_mat().add_(1.0)
    assert decoded_u8(g) is None
    assert decoded_u8(A.HFlip().transform(_features(1)[0])) is None


def test_chain_recognition():
    from bigdl.transform.vision.image import augmentation as A
    from bigdl.transform.vision.image.convertor import LoweredTail, MatToTensor, MTImageFeatureToBatch
    from bigdl.transform.vision.image.image_feature import Pipeline
    from bigdl.utils.random import RNG
    norm = A.ChannelScaledNormalizer(104, 117, 123, 0.0078125)
    accepted = [
        None, A.RandomAlterAspect(crop_length=16), _chain(), _chain() >> MatToTensor(),
        A.RandomCropper(16, 16, True), A.CenterCrop(16, 16) >> A.HFlip() >> A.ChannelNormalize(1, 2, 3, 4, 5, 6),
        A.RandomCrop(16, 16) >> norm, A.HFlip(), norm >> MatToTensor(), MatToTensor(),
        Pipeline([A.Brightness(-1, 1), Pipeline([A.RandomAlterAspect(crop_length=16), A.RandomCropper(16, 16, False)]),
                  norm]),
        A.Resize(30, 30) >> A.ColorJitter() >> A.RandomCrop(16, 16) >> A.ChannelNormalize(1, 2, 3),
    ]
    for t in accepted:
        RNG.setSeed(3)
        mt = MTImageFeatureToBatch(16, 16, 4, transformer=t, device="cpu", device_augment=True)
        b = next(iter(mt(_features(4))))
        assert b.getInput().shape == (4, 3, 16, 16) and bool(torch.isfinite(b.getInput()).all())
    low = LoweredTail(A.Resize(30, 30) >> A.ColorJitter() >> A.RandomCrop(16, 16) >> norm)
    assert [type(t).__name__ for t in low.prefix] == ["Resize", "ColorJitter"] and low.cropper is not None
    for bad, name in [(_chain() >> A.Resize(16, 16), "Resize"), (A.HFlip() >> A.ColorJitter(), "ColorJitter"),
                      (norm >> A.RandomCropper(16, 16, True), "RandomCropper"),
                      (A.RandomCropper(16, 16, True) >> A.RandomAlterAspect(crop_length=16), "RandomAlterAspect")]:
        with pytest.raises(ValueError, match=name):
            MTImageFeatureToBatch(16, 16, 4, transformer=bad, device="cpu", device_augment=True)
    with pytest.raises(ValueError, match="compose"):
        MTImageFeatureToBatch(16, 16, 4, transformer=A.RandomAlterAspect(crop_length=16) >>
                              A.RandomCropper(12, 12, True), device="cpu", device_augment=True)
    with pytest.raises(ValueError, match="compose"):
        MTImageFeatureToBatch(12, 12, 4, transformer=A.RandomAlterAspect(crop_length=16), device="cpu",
                              device_augment=True)
    with pytest.raises(ValueError, match="LINEAR or CUBIC"):
        MTImageFeatureToBatch(16, 16, 4, transformer=A.RandomAlterAspect(interp_mode="AREA", crop_length=16),
                              device="cpu", device_augment=True)


def test_crop_only_lowering_equals_host_path():
    """No resize in the tail: the lowered batch is the host path's batch (same draws, identity resample)."""
    from bigdl.transform.vision.image import augmentation as A
    from bigdl.transform.vision.image.convertor import MTImageFeatureToBatch
    from bigdl.utils.random import RNG
    for t in (lambda: A.RandomCropper(18, 17, True, "Random") >> A.ChannelNormalize(100, 110, 120, 50, 60, 70),
              lambda: A.CenterCrop(19, 18) >> A.HFlip(), lambda: A.RandomCrop(18, 18)):
        outs = []
        for dev_aug in (False, True):
            RNG.setSeed(11)
            mt = MTImageFeatureToBatch(16, 16, 8, transformer=t(), device="cpu", device_augment=dev_aug,
                                       to_rgb=True, mean=(1, 2, 3), std=(1, 2, 4), num_threads=1)
            outs.append(next(iter(mt(_features()))).getInput())
        assert float((outs[0] - outs[1]).abs().max()) <= 1e-5


def test_default_path_unchanged():
    """``device_augment=False``: the chain on the host, then crop / mirror / normalise of the stacked crops."""
    from bigdl.transform.vision.image.convertor import MTImageFeatureToBatch
    from bigdl.utils.random import RNG
    RNG.setSeed(9)
    chain = _chain()
    mats = [chain.transform(f).opencv_mat() for f in _features()]
    fl = [1 if RNG.uniform(0, 1) < 0.5 else 0 for _ in mats]
    want = R.image_crop_flip_norm(torch.stack(mats), [0] * 8, [0] * 8, fl, 16, 16, (3, 2, 1), (4, 2, 1), False)
    RNG.setSeed(9)
    mt = MTImageFeatureToBatch(16, 16, 8, transformer=_chain(), device="cpu", to_rgb=False, mean=(1, 2, 3),
                               std=(1, 2, 4), mirror=True, num_threads=1)
    assert mt.lowered is None
    assert torch.equal(next(iter(mt(_features()))).getInput(), want)


# ------------------------------------------------------------------------------------------- 5, 6: raw loader
def _raw_data(n=32, h=24, w=24, c=3):
    rng = np.random.RandomState(4)
    return rng.randint(0, 256, size=(n, h, w, c)).astype(np.uint8), np.arange(n, dtype=np.float32) + 1


def _pull(ld, nbatch):
    """[(input, target, slot pixels, descriptor rows)] — the slot blocks are copied before the next call
    hands the slot back to the workers."""
    out = []
    for i in range(nbatch):
        b = ld.next_batch()
        s = i % len(ld._x)
        r = b.getInput().shape[0]
        out.append((b.getInput(), b.getTarget(), ld._x[s][:r].clone(), ld._d[s][:r].clone()))
    return out


def test_raw_loader_train():
    from bigdl.runtime import NativeBatchLoader
    x, y = _raw_data()
    mean, std = [104.0, 117.0, 123.0], [58.0, 57.0, 59.0]
    runs = []
    for t in (1, 4):
        ld = NativeBatchLoader(x, y, 8, crop=(16, 16), flip=True, train=True, mean=mean, std=std, layout="NHWC",
                               seed=7, threads=t, prefetch=3, device="cpu", raw=True, alter_aspect=(0.08, 1, 0.75),
                               interp="CUBIC")
        runs.append(_pull(ld, 250))
        ld.close()
    for a, b in zip(*runs):  # a pure function of (seed, batch): independent of the thread count
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    d = torch.cat([r[3] for r in runs[0]]).numpy()
    assert d.shape == (2000, 8) and (d[:, 1] == 24).all() and (d[:, 2] == 24).all()
    assert (d[:, 0] == np.tile(np.arange(8) * 24 * 24 * 3, 250)).all()
    assert (d[:, 3] >= 0).all() and (d[:, 4] >= 0).all() and (d[:, 5] > 0).all() and (d[:, 6] > 0).all()
    assert (d[:, 3] + d[:, 5] <= 24).all() and (d[:, 4] + d[:, 6] <= 24).all()
    ratio = d[:, 5] * d[:, 6] / (24.0 * 24.0)
    assert ratio.min() > 0.08 - 1 / 24 and ratio.max() <= 1.0
    assert set(d[:, 7].tolist()) == {0, 1}
    assert (d[:, 5] > d[:, 6]).any() and (d[:, 5] < d[:, 6]).any()
    for xin, tgt, px, desc in runs[0][:5]:
        idx = tgt.long() - 1
        assert torch.equal(px, torch.from_numpy(x)[idx])  # row r holds images[perm[off + r]]
        want = R.image_resample_norm(px.reshape(-1), desc[:, 3:7], desc[:, 7], 16, 16, mean, std, False, "CUBIC",
                                     sizes=torch.tensor([[24, 24, 3]] * 8), offsets=desc[:, 0])
        assert xin.shape == (8, 3, 16, 16) and torch.equal(xin, want)
    labels = torch.cat([r[1] for r in runs[0][:4]])
    assert sorted(labels.tolist()) == list(range(1, 33))  # one epoch = a permutation


def test_raw_loader_fixed_crop_and_eval():
    from bigdl.runtime import NativeBatchLoader
    x, y = _raw_data()
    mean, std = [10.0, 20.0, 30.0], [2.0, 4.0, 8.0]
    ld = NativeBatchLoader(x, y, 8, crop=(16, 12), flip=True, train=True, mean=mean, std=std, seed=3, threads=3,
                           device="cpu", raw=True)
    got = _pull(ld, 40)
    d = torch.cat([r[3] for r in got]).numpy()
    ld.close()
    host = NativeBatchLoader(x, y, 8, crop=(16, 12), flip=True, train=True, mean=mean, std=std, seed=3, threads=3,
                             device="cpu")
    for r in got[:6]:  # the same stream gives the host mode's crop origins and flips: the same batches
        b = host.next_batch()
        np.testing.assert_allclose(r[0].numpy(), b.getInput().numpy(), rtol=1e-6, atol=1e-6)
        assert torch.equal(r[1], b.getTarget())
    host.close()
    assert (d[:, 5] == 16).all() and (d[:, 6] == 12).all() and set(d[:, 7].tolist()) == {0, 1}
    assert d[:, 3].min() == 0 and d[:, 3].max() == 8 and d[:, 4].min() == 0 and d[:, 4].max() == 12
    for alter in (None, (0.08, 1, 0.75)):  # eval: the centred rectangle, no flip, whatever the train recipe
        ld = NativeBatchLoader(x, y, 8, crop=(16, 12), flip=True, train=False, mean=mean, std=std, shuffle=False,
                               threads=2, device="cpu", raw=True, alter_aspect=alter)
        xin, tgt, px, desc = _pull(ld, 1)[0]
        ld.close()
        assert (desc[:, 3:].numpy() == np.array([4, 6, 16, 12, 0])).all()
        ref = (x[:8, 4:20, 6:18, :].astype(np.float32) - np.array(mean, np.float32)) / np.array(std, np.float32)
        np.testing.assert_allclose(xin.numpy(), ref.transpose(0, 3, 1, 2), rtol=1e-6)
        assert xin.is_contiguous() and tgt.tolist() == y[:8].tolist()  # NCHW layout on request
    with pytest.raises(ValueError):
        NativeBatchLoader(x, y, 8, crop=(16, 12), pad=2, device="cpu", raw=True)
    with pytest.raises(ValueError):
        NativeBatchLoader(x, y, 8, crop=(30, 12), device="cpu", raw=True)


def test_raw_loader_thread_sanitizer_stress(tmp_path):
    """Raw mode under ThreadSanitizer and ASan/UBSan, as tests/test_native_loader.py does for the host mode:
    a stand-alone program, nothing loaded into Python."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    srcs = [os.path.join(ROOT, "tools", "native_tests", "loader_raw_stress.cpp"),
            os.path.join(ROOT, "bigdl-1_amd", "bigdl", "runtime", "csrc", "batch_loader.cpp")]
    for san in ("thread", "address,undefined"):
        exe = str(tmp_path / ("raw_stress_" + san.split(",")[0]))
        subprocess.run([gxx, "-O1", "-g", f"-fsanitize={san}", "-pthread"] + srcs + ["-o", exe], check=True,
                       capture_output=True, timeout=240)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "raw loader stress ok" in r.stdout, (r.returncode, r.stderr[-3000:])
        assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr
        assert "runtime error" not in r.stderr


# ------------------------------------------------------------------------------------------- 7: training CLI
def test_imagenet_cli_device_augment():
    from bigdl.models.train import imagenet
    base = ["--synthetic", "64", "-b", "8", "-e", "1", "--maxIteration", "2", "--net", "resnet", "--depth", "18",
            "--classes", "10", "--dtype", "fp32", "--threads", "2", "--seed", "5"]
    off = [imagenet.main(base)["Loss"] for _ in range(2)]
    assert off[0] == off[1] and np.isfinite(off[0])  # flags off: the host loader, the same loss every run
    on = imagenet.main(base + ["--deviceAugment", "--alterAspect"])
    assert on["neval"] == 3 and np.isfinite(on["Loss"]) and on["Loss"] != off[0]


def test_image_loader_flags_pick_the_loader():
    import argparse
    from bigdl.models.train.common import image_loader
    x, y = _raw_data()
    mk = lambda **kw: argparse.Namespace(seed=1, threads=2, **kw)  # noqa: E731
    for args, train, raw, alter in [(mk(), True, False, False), (mk(deviceAugment=True, alterAspect=False), True,
                                                                  True, False),
                                    (mk(deviceAugment=False, alterAspect=True), True, True, True),
                                    (mk(deviceAugment=False, alterAspect=True), False, True, False)]:
        ld = image_loader(x, y, 8, (16, 16), train, [0.0] * 3, [1.0] * 3, args)
        d = _pull(ld, 3)[-1][3] if raw else None
        assert ld.raw == raw
        if raw:
            assert bool(((d[:, 5] != 16) | (d[:, 6] != 16)).any()) == alter
        ld.close()
