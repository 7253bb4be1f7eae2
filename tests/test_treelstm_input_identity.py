"""``BinaryTreeLSTM.backward`` finds the native forward's saves by the input's tensors, not by the Table around
them: a caller may wrap the same tensors in a new Table for the backward (tests/test_treelstm_native.py does), and
whether a new Table gets the id of the forward's freed one is the allocator's choice.  Here the forward's Table is
kept alive, so the backward's Table has another id for certain; the embedding gradient must still be the native
one, bit for bit (the torch bf16 path rounds elsewhere)."""
import pytest
import torch

from test_tree_lstm import TREE1, TREE2


@pytest.mark.gpu
def test_backward_with_a_new_table_stays_native():
    from bigdl import ops
    from bigdl.nn import BinaryTreeLSTM
    from bigdl.utils.engine import Engine
    from bigdl.utils.table import Table
    Engine.init(device="cuda:0")
    trees = torch.tensor([TREE1, TREE2], dtype=torch.float32).cuda()
    B, N, L = trees.shape[0], trees.shape[1], int(trees[..., 2].max())
    m = BinaryTreeLSTM(10, 22).to(device="cuda")
    m.training()
    x, gy = torch.randn(B, L, 10).to(torch.bfloat16).cuda(), torch.randn(B, N, 22).to(torch.bfloat16).cuda()
    ops.reset_fallbacks()
    same = Table(x, trees)
    m.forward(same)
    gx_same = m.backward(same, gy)[1].clone()
    kept = Table(x, trees)
    m.forward(kept)
    gx_new = m.backward(Table(x, trees), gy)[1]
    assert ops.fallback_counts() == {}
    assert torch.equal(gx_new, gx_same)
