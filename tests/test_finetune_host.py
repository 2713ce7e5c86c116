"""CPU tests of the fine-tuning head (torch_cfd_amd.finetune.OutConvFT): buffers, state_dict keys, the placement of the old
layer's blocks in the widened convolution (golden from the reference, tests/golden/make_golden_finetune.py) and the
latent hooks of FNOBase."""
import math

import numpy as np
import pytest
import torch

from torch_cfd_amd.finetune import OutConvFT


def test_state_dict_keys_and_buffers_match_the_reference(golden):
    g = golden("finetune_weights.npz")
    torch.set_default_dtype(torch.float64)
    head = OutConvFT(4, 4, 2, n_grid=16, delta=1)
    head._update_spectral_conv_weights(6, 6, 3, device="cpu")
    assert list(head.state_dict().keys()) == list(g["state_dict_keys"])
    shapes = [list(head.state_dict()[k].shape) for k in ("lap", "kx", "ky", "dealias_filter")]
    assert shapes == g["buffer_shapes"].tolist()
    assert (head.mode_x, head.mode_y, head.mode_t) == tuple(g["modes"].tolist())


def test_buffers_quirks():
    torch.set_default_dtype(torch.float64)
    n = 32
    head = OutConvFT(4, 4, 2, n_grid=n, delta=1, batch_size=3)
    assert head.lap.shape == head.kx.shape == head.ky.shape == head.dealias_filter.shape == (3, n, n // 2 + 1)
    assert torch.all(head.lap[:, 0, 0] == 1)
    # diam = 1: |k| / diam <= (2/3)(n // 2) is a real 2/3 mask
    k = np.fft.fftfreq(n, d=1.0 / n)
    keep = np.abs(k) <= (2 / 3) * (n // 2)
    expect = np.logical_and(keep[:, None], keep[None, : n // 2 + 1]).astype(np.float64)
    assert np.array_equal(head.dealias_filter[0].numpy(), expect) and expect.mean() < 1
    # diam = 2 pi (the notebook): every |k| / diam is below the cut, the mask is all ones
    nb = OutConvFT(4, 4, 2, n_grid=n, delta=1, diam=2 * math.pi)
    assert torch.all(nb.dealias_filter == 1)
    assert OutConvFT(4, 4, 2, n_grid=n, dealias=False).dealias_filter.item() is True


def test_update_spectral_conv_weights_block_placement(golden):
    g = golden("finetune_weights.npz")
    torch.set_default_dtype(torch.float64)
    old = OutConvFT(4, 4, 2, n_grid=16, delta=1)
    for k in range(4):
        old.conv.weight[k].data.copy_(torch.from_numpy(g[f"old_weight{k}"]))
        old.conv.bias[k].data.copy_(torch.from_numpy(g[f"old_bias{k}"]))
    head = OutConvFT(4, 4, 2, n_grid=16, delta=1)
    head._update_spectral_conv_weights(6, 6, 3, device="cpu", model=old)
    for k in range(4):
        ref_w, ref_b = g[f"new_weight{k}"], g[f"new_bias{k}"]
        new_w, new_b = head.conv.weight[k].data.numpy(), head.conv.bias[k].data.numpy()
        assert new_w.shape == ref_w.shape and new_b.shape == ref_b.shape
        # the copied blocks: corner ix + 2 iy at [:4] / [-4:] x [:4] / [-4:] x [:2], equal to the reference's
        ix, iy = k % 2, k // 2
        sx = slice(0, 4) if ix == 0 else slice(-4, None)
        sy = slice(0, 4) if iy == 0 else slice(-4, None)
        np.testing.assert_array_equal(new_w[..., sx, sy, :2, :], ref_w[..., sx, sy, :2, :])
        np.testing.assert_array_equal(new_w[..., sx, sy, :2, :], g[f"old_weight{k}"])
        np.testing.assert_array_equal(new_b[..., sx, sy, :2, :], ref_b[..., sx, sy, :2, :])
        # the bias elsewhere is zero, the weights elsewhere are Xavier-uniform with gain 1e-6 (tiny), as the reference's
        rest = np.ones(new_w.shape, bool)
        rest[..., sx, sy, :2, :] = False
        assert np.all(np.abs(new_w[rest]) < 1e-6) and np.all(np.abs(ref_w[rest]) < 1e-6)
        rest_b = np.ones(new_b.shape, bool)
        rest_b[..., sx, sy, :2, :] = False
        assert np.all(new_b[rest_b] == 0) and np.all(ref_b[rest_b] == 0)


def test_reset_parameters_xavier_gain():
    from torch_cfd_amd.fno import SpectralConvT

    conv = SpectralConvT(1, 1, 6, 6, 3, bias=True)
    conv._reset_parameters()
    for p in conv.bias:
        assert torch.all(p == 0)
    fan = 6 * 6 * 3 * 2
    bound = 1e-6 * math.sqrt(6.0 / (2 * fan))
    for p in conv.weight:
        assert p.abs().max() <= bound and p.abs().max() > 0


def test_latent_hooks_record_detached_outputs():
    from torch_cfd_amd.fno import FNOBase

    class Tiny(FNOBase):
        def __init__(self):
            super().__init__()
            self.reduction = torch.nn.Linear(3, 1)
            self.blocks = torch.nn.ModuleList([torch.nn.Linear(3, 3), torch.nn.Linear(3, 3)])

        def forward(self, x):
            for b in self.blocks:
                x = b(x)
            return self.reduction(x)

    m = Tiny()
    m.add_latent_hook("reduction")
    m.add_latent_hook("blocks")
    x = torch.randn(2, 3, requires_grad=True)
    y = m(x)
    assert torch.equal(m.latent_tensors["reduction"], y.detach()) and not m.latent_tensors["reduction"].requires_grad
    assert set(m.latent_tensors) >= {"reduction", "blocks_0", "blocks_1"}
