"""Device-side augmentation on the GPU: the crop → resample → mirror → normalise → cast kernel
(``csrc/image_aug.hip``) against the fp64 oracle of ``tests/test_image_augment_cpu.py``, and the two public
paths that use it (``MTImageFeatureToBatch(device_augment=True)``, ``NativeBatchLoader(raw=True)``).

Bound (the convention of tests/test_optim_fused.py): ``max|kernel − fp64| ≤ 4·E_torch + 1e-6``, E_torch the
error of the fp32 torch operator on the same inputs.  The kernel takes its sample phases from integers and
forms its weights in fp64, so it should land well inside; every test prints its figures
(profiles/image_aug_errors.txt keeps one run of them).
"""
import numpy as np
import pytest
import torch

from test_image_augment_cpu import MEAN, OUT_SIZES, STD, case, expected, oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bigdl.ops import native_has
    assert native_has("image_resample_norm"), "image_resample_norm kernel missing"


def _kernel(C, out_hw, src_float, interp, to_rgb, out_dtype=torch.float32, **kw):
    from bigdl.ops import native_ops as NO
    _, packed, sizes, offsets, rects, flip, _ = case(C, out_hw, src_float)
    return NO.image_resample_norm(packed.cuda(), rects, flip, out_hw[0], out_hw[1], MEAN, STD, to_rgb, interp,
                                  out_dtype, sizes=sizes, offsets=offsets, **kw)


def _check(tag, got, want, e_torch):
    err = float(np.abs(got.double().cpu().numpy() - want).max())
    bound = 4 * e_torch + 1e-6
    print(f"image_aug_error {tag} torch_fp32={e_torch:.3e} kernel={err:.3e} kernel/bound={err / bound:.3f}")
    assert err <= bound, (tag, err, bound)


@pytest.mark.parametrize("interp", ["LINEAR", "CUBIC"])
@pytest.mark.parametrize("out_hw", OUT_SIZES)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_kernel_against_fp64(C, out_hw, interp):
    from bigdl.ops import native_ops as NO
    for src_float in (False, True):
        for to_rgb in (False, True):
            want, e = expected(C, out_hw, src_float, interp, to_rgb)
            got = _kernel(C, out_hw, src_float, interp, to_rgb)
            assert tuple(got.shape) == want.shape and got.permute(0, 2, 3, 1).is_contiguous()
            assert NO.image_resample_last_variant() == "staged"
            _check(f"C={C} out={out_hw} src={'f32' if src_float else 'u8'} {interp} to_rgb={int(to_rgb)}",
                   got, want, e)


@pytest.mark.parametrize("interp", ["LINEAR", "CUBIC"])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_bf16_output_is_rounded_fp32_output(C, interp):
    for out_hw in OUT_SIZES:
        for src_float in (False, True):
            f = _kernel(C, out_hw, src_float, interp, True)
            h = _kernel(C, out_hw, src_float, interp, True, torch.bfloat16)
            assert h.dtype == torch.bfloat16 and torch.equal(f.to(torch.bfloat16), h)


@pytest.mark.parametrize("interp", ["LINEAR", "CUBIC"])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_identity_rectangles_give_crop_flip_norm_bits(out_dtype, interp):
    from bigdl.ops import native_ops as NO
    rng = np.random.default_rng(5)
    src = torch.from_numpy(rng.integers(0, 256, size=(5, 21, 23, 3), dtype=np.uint8)).cuda()
    oy, ox, fl = [0, 3, 9, 5, 1], [7, 0, 2, 6, 3], [0, 1, 1, 0, 1]
    rects = torch.tensor([[y, x, 12, 16] for y, x in zip(oy, ox)])
    for to_rgb in (False, True):
        a = NO.image_resample_norm(src, rects, fl, 12, 16, MEAN, STD, to_rgb, interp, out_dtype)
        b = NO.image_crop_flip_norm(src, torch.tensor(oy), torch.tensor(ox), torch.tensor(fl), 12, 16, MEAN, STD,
                                    to_rgb, out_dtype)
        assert torch.equal(a, b)


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("variant", ["staged", "direct"])
def test_out_argument_leaves_guards_untouched(variant, out_dtype):
    C, out_hw = 3, (20, 24)
    B = case(C, out_hw, False)[4].shape[0]
    outs = []
    for _ in range(2):
        big = torch.full((B + 2, out_hw[0], out_hw[1], C), -777.0, dtype=out_dtype, device="cuda")
        got = _kernel(C, out_hw, False, "CUBIC", False, out_dtype, out=big[1:-1].permute(0, 3, 1, 2),
                      variant=variant)
        torch.cuda.synchronize()
        assert got.data_ptr() == big[1].data_ptr()
        assert bool((big[0] == -777.0).all()) and bool((big[-1] == -777.0).all())
        assert not bool((big[1:-1] == -777.0).any())
        outs.append(big.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("interp", ["LINEAR", "CUBIC"])
def test_direct_variant(interp):
    """A 6×3000×3 image is a few KB but wider than the staged variant's LDS budget: the host picks the direct
    gather.  On a narrow batch both variants run the same fma sequence on the same taps, so they agree to
    the last bit."""
    from bigdl.ops import native_ops as NO
    from bigdl.ops import reference as R
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, size=(1, 6, 3000, 3), dtype=np.uint8)
    rects, fl = torch.tensor([[0, 0, 6, 3000]]), [1]
    want = oracle([img[0]], [(0, 0, 0, 6, 3000, 1)], 16, 16, MEAN, STD, False, interp).transpose(0, 3, 1, 2)
    ref = R.image_resample_norm(torch.from_numpy(img), rects, fl, 16, 16, MEAN, STD, False, interp)
    got = NO.image_resample_norm(torch.from_numpy(img).cuda(), rects, fl, 16, 16, MEAN, STD, False, interp)
    assert NO.image_resample_last_variant() == "direct"
    _check(f"direct 6x3000 {interp}", got, want, float(np.abs(ref.double().numpy() - want).max()))
    with pytest.raises(ValueError):
        NO.image_resample_norm(torch.from_numpy(img).cuda(), rects, fl, 16, 16, MEAN, STD, False, interp,
                               variant="staged")
    for C in (1, 3, 4):
        for src_float in (False, True):
            for dt in (torch.float32, torch.bfloat16):
                a = _kernel(C, (20, 24), src_float, interp, True, dt, variant="staged")
                assert NO.image_resample_last_variant() == "staged"
                b = _kernel(C, (20, 24), src_float, interp, True, dt, variant="direct")
                assert NO.image_resample_last_variant() == "direct"
                assert torch.equal(a, b)


def _bf16_ulp_apart(a, b):
    """Largest distance of two bf16 tensors in units of the bf16 grid (ordered-integer view)."""
    ia, ib = (t.contiguous().view(torch.int16).to(torch.int32) for t in (a, b))
    ia, ib = (torch.where(i < 0, -(i & 0x7fff), i) for i in (ia, ib))
    return int((ia - ib).abs().max())


@pytest.mark.parametrize("interp", ["LINEAR", "CUBIC"])
def test_mt_batch_device_augment_matches_cpu(interp):
    from test_image_augment_cpu import _features
    from bigdl import ops
    from bigdl.transform.vision.image import augmentation as A
    from bigdl.transform.vision.image.convertor import MTImageFeatureToBatch
    from bigdl.utils.random import RNG

    def run(device, dtype):
        RNG.setSeed(21)
        chain = (A.RandomAlterAspect(interp_mode=interp, crop_length=16) >> A.RandomCropper(16, 16, True, "Random")
                 >> A.ChannelScaledNormalizer(104, 117, 123, 0.0078125))
        mt = MTImageFeatureToBatch(16, 16, 8, transformer=chain, device=device, device_augment=True, to_rgb=False,
                                   out_dtype=dtype)
        b = next(iter(mt(_features())))
        return b.getInput().cpu(), b.getTarget().cpu()

    ops.reset_fallbacks()
    for dtype in (torch.float32, torch.bfloat16):
        (xc, yc), (xg, yg) = run("cpu", dtype), run("cuda", dtype)
        assert torch.equal(yc, yg) and xg.shape == (8, 3, 16, 16) and xg.dtype == dtype
        if dtype == torch.float32:
            # both are within their own error of the fp64 value: E_torch for the CPU arm, the kernel's bound
            # 4·E_torch + 1e-6 for the GPU arm; E_torch itself is taken against the oracle on these inputs
            feats = _features()
            RNG.setSeed(21)
            low = MTImageFeatureToBatch(16, 16, 8, transformer=A.RandomAlterAspect(interp_mode=interp,
                                        crop_length=16) >> A.RandomCropper(16, 16, True, "Random"), device="cpu",
                                        device_augment=True).lowered
            rows = []
            for k, f in enumerate(feats):
                (y, x, ch, cw), _, fl = low.draw(f.get_height(), f.get_width(), 3)
                rows.append((k, y, x, ch, cw, int(fl)))
            want = oracle([f.opencv_mat().numpy() for f in feats], rows, 16, 16, (123.0, 117.0, 104.0),
                          (128.0,) * 3, False, interp).transpose(0, 3, 1, 2)
            e_torch = float(np.abs(xc.double().numpy() - want).max())
            _check(f"mt_batch {interp}", xg, want, e_torch)
            assert float((xc - xg).abs().max()) <= 5 * e_torch + 1e-6
        else:
            assert _bf16_ulp_apart(xc, xg) <= 1
    assert ops.fallback_counts() == {}


def test_raw_loader_device_matches_cpu():
    from bigdl.runtime import NativeBatchLoader
    rng = np.random.RandomState(4)
    x = rng.randint(0, 256, size=(32, 24, 24, 3)).astype(np.uint8)
    y = np.arange(32, dtype=np.float32) + 1
    mean, std = [104.0, 117.0, 123.0], [58.0, 57.0, 59.0]

    def mk(device, dtype):
        return NativeBatchLoader(x, y, 8, crop=(16, 16), flip=True, train=True, mean=mean, std=std, dtype=dtype,
                                 layout="NHWC", seed=9, threads=3, device=device, raw=True,
                                 alter_aspect=(0.08, 1, 0.75), interp="CUBIC")
    cpu, gpu, gpu16 = mk("cpu", torch.float32), mk("cuda", torch.float32), mk("cuda", torch.bfloat16)
    for i in range(3):
        bc = cpu.next_batch()
        desc = cpu._d[i % len(cpu._d)][:8].clone()
        bg, bh = gpu.next_batch(), gpu16.next_batch()
        torch.cuda.synchronize()
        rows = [(int(bc.getTarget()[r]) - 1,) + tuple(int(v) for v in desc[r, 3:8]) for r in range(8)]
        want = oracle(list(x), rows, 16, 16, mean, std, False, "CUBIC").transpose(0, 3, 1, 2)
        e_torch = float(np.abs(bc.getInput().double().numpy() - want).max())
        _check(f"raw_loader batch {i}", bg.getInput(), want, e_torch)
        assert torch.equal(bc.getTarget(), bg.getTarget().cpu()) and torch.equal(bc.getTarget(), bh.getTarget().cpu())
        xh = bh.getInput()
        assert xh.dtype == torch.bfloat16 and xh.shape == (8, 3, 16, 16)
        assert xh.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(xh, bg.getInput().to(torch.bfloat16))
    for ld in (cpu, gpu, gpu16):
        ld.close()
