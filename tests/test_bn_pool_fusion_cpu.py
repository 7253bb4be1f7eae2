"""bigdl.fusion.bnpool on the CPU: fuse() / unfuse() flag exactly the BN → ReLU → 3×3 / stride-2 max-pool
pattern, the reference path computes the same with the flag on and off, and the reference
implementations of the deferred contract (ops.reference: bn_maxpool_forward, PoolGrad,
batchnorm_backward_pool, relu_mask) are the composition of the plain BN and pool reference ops."""
import copy

import pytest
import torch


def _seq(pool, relu=True, bn_format="NCHW"):
    from bigdl.nn import Sequential, SpatialConvolution, SpatialBatchNormalization, ReLU
    s = Sequential().add(SpatialConvolution(3, 8, 3, 3, 1, 1, 1, 1))
    s.add(SpatialBatchNormalization(8, data_format=bn_format))
    if relu:
        s.add(ReLU(True))
    return s.add(pool).add(SpatialConvolution(8, 4, 1, 1))


def _pool(*a, **kw):
    from bigdl.nn import SpatialMaxPooling
    return SpatialMaxPooling(*a, **kw)


def test_fuse_flags_the_pattern_and_unfuse_clears_it():
    from bigdl.nn.fusion import fuse, unfuse
    from bigdl.nn.layers.normalization import BatchNormalization
    for pad in (0, 1):
        m = _seq(_pool(3, 3, 2, 2, pad, pad))
        fuse(m)
        bn, pool = m.modules[1], m.modules[3]
        assert bn._fused_relu and bn._pool_consumer is pool and pool._bn_producer is bn
        unfuse(m)
        assert bn._pool_consumer is None and pool._bn_producer is None and pool._bn_in is None
        fuse(m, bnpool=False)
        assert bn._pool_consumer is None and pool._bn_producer is None
    others = [_seq(_pool(2, 2, 2, 2)), _seq(_pool(3, 3, 1, 1, 1, 1)), _seq(_pool(3, 3, 2, 2, 1, 1).ceil()),
              _seq(_pool(3, 3, 2, 2, 1, 1), relu=False), _seq(_pool(3, 3, 2, 2, 0, 1, format="NHWC")),
              _seq(_pool(5, 5, 2, 2, 2, 2))]
    for m in others:
        fuse(m)
        for mod in m.flattened_modules():
            if isinstance(mod, BatchNormalization):
                assert mod._pool_consumer is None
            if type(mod).__name__ == "SpatialMaxPooling":
                assert mod._bn_producer is None


def test_bnrelu_off_leaves_the_pool_alone():
    from bigdl.nn.fusion import fuse
    m = _seq(_pool(3, 3, 2, 2, 1, 1))
    fuse(m, bnrelu=False)
    assert m.modules[1]._pool_consumer is None and m.modules[3]._bn_producer is None


def test_reference_path_same_with_flag_on_and_off():
    from bigdl.nn.fusion import fuse
    from bigdl.utils.random import RNG
    RNG.setSeed(11)
    base = _seq(_pool(3, 3, 2, 2, 1, 1))
    base.training()
    x = torch.randn(3, 3, 9, 10)
    out = []
    for on in (False, True):
        m = copy.deepcopy(base)
        fuse(m, bnpool=on)
        assert (m.modules[1]._pool_consumer is not None) == on
        m.zeroGradParameters()
        y = m.forward(x)
        gi = m.backward(x, torch.ones_like(y) * torch.linspace(-1, 1, y.numel()).view(y.shape))
        out.append((y.clone(), gi.clone(), [g.clone() for g in m.parameters()[1]]))
    (ya, ga, pa), (yb, gb, pb) = out
    assert torch.equal(ya, yb) and torch.equal(ga, gb)
    for u, v in zip(pa, pb):
        assert torch.equal(u, v)


def _bn(C=8, H=9, W=10, seed=0):
    from bigdl.ops import reference as R
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, C, H, W, generator=g).contiguous(memory_format=torch.channels_last)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    coef = torch.empty(2 * C)
    y, mean, invstd = R.batchnorm_forward_train(x, gamma, beta, None, None, 0.1, 1e-5, relu=True, coef_out=coef)
    return x, gamma, coef, y, mean, invstd


@pytest.mark.parametrize("pad", [0, 1])
def test_reference_contract_is_the_composition(pad):
    from bigdl.ops import reference as R
    x, gamma, coef, y, mean, invstd = _bn()
    k, s, p = (3, 3), (2, 2), (pad, pad)
    b = R.BNOut(x, coef, relu=True)
    torch.testing.assert_close(b.dense(), y, rtol=1e-5, atol=1e-5)
    yd = b.dense()
    yp, idx = R.maxpool2d_forward(yd, k, s, p, False)
    fp, fidx = R.bn_maxpool_forward(b, k, s, p, False)
    assert torch.equal(fp, yp) and torch.equal(fidx, idx)
    gp = torch.randn(yp.shape, generator=torch.Generator().manual_seed(4))
    pg = R.PoolGrad(gp, fidx, k, s, p, b)
    gd = R.maxpool2d_backward(gp, yd, idx, k, s, p, False)
    assert torch.equal(R.as_dense(pg), gd) and pg.shape == tuple(x.shape)

    def acc():
        return [torch.zeros(x.shape[1]) for _ in range(3)]
    a, c = acc(), acc()
    gx = R.batchnorm_backward_pool(pg, x, gamma, mean, invstd, fcoef=coef, gg_acc=a[0], gb_acc=a[1], scale=0.5,
                                   cbias_acc=a[2], cbias_scale=1.0)
    gx0, _ = R.batchnorm_backward(gd, x, gamma, mean, invstd, y=yd, relu=True, gg_acc=c[0], gb_acc=c[1], scale=0.5,
                                  cbias_acc=c[2], cbias_scale=1.0)
    assert torch.equal(gx, gx0)
    for u, v in zip(a, c):
        assert torch.equal(u, v)


def test_relu_mask_sources_agree():
    from bigdl.ops import reference as R
    x, gamma, coef, _, mean, invstd = _bn(C=16, seed=2)
    y = R.BNOut(x, coef, relu=True).dense()
    bits = torch.empty(x.numel() // 8, dtype=torch.uint8)
    pos = (y.permute(0, 2, 3, 1).reshape(-1, 8) > 0).to(torch.int32)
    bits.copy_((pos * (2 ** torch.arange(8, dtype=torch.int32)).view(1, 8)).sum(1).to(torch.uint8))
    want = y > 0
    assert 0.2 < float(want.float().mean()) < 0.8
    assert torch.equal(R.relu_mask(x, fcoef=coef), want)
    assert torch.equal(R.relu_mask(x, mask_bits=bits), want)
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(9))
    g0, _ = R.batchnorm_backward(gy, x, gamma, mean, invstd, y=y, relu=True)
    for kw in (dict(fcoef=coef), dict(mask_bits=bits)):
        g1, _ = R.batchnorm_backward(gy, x, gamma, mean, invstd, relu=True, **kw)
        assert torch.equal(g1, g0)


def test_pool_layer_takes_a_deferred_input_on_the_reference_path():
    """The layer logic itself: a BNOut in, the pooled BN + ReLU out; the backward answers with a PoolGrad
    for the object the forward consumed and with a dense gradient for any other."""
    from bigdl.ops import reference as R
    x, gamma, coef, y, mean, invstd = _bn(seed=5)
    b = R.BNOut(x, coef, relu=True)
    pool, plain = _pool(3, 3, 2, 2, 1, 1), _pool(3, 3, 2, 2, 1, 1)
    pool.training()
    plain.training()
    out = pool.forward(b)
    want = plain.forward(b.dense())
    assert torch.equal(out, want)
    gp = torch.randn(out.shape, generator=torch.Generator().manual_seed(6))
    pg = pool.backward(b, gp)
    assert isinstance(pg, R.PoolGrad) and pg.src is b
    gd = plain.backward(b.dense(), gp)
    assert torch.equal(pg.dense(), gd)
    again = R.BNOut(x, coef, relu=True)
    assert torch.equal(pool.updateGradInput(again, gp), gd)
    pool.evaluate()
    assert torch.equal(pool.forward(b), want) and pool._bn_in is None
