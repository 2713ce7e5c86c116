"""The FNO3d baseline restated with plain torch ops: ``rfftn`` / four-corner einsum / ``irfftn`` for the Fourier layers, channel
einsums for the 1x1x1 convolutions, ``F.pad`` (circular) for the padding.  It takes a ``state_dict`` (the reference's key names),
runs on the CPU and on the GPU, is differentiable by torch autograd, and reads nothing but its arguments: the yardstick of
``torch_cfd_amd.fno.FNO3d`` at sizes too big for a fixture, and the pure-torch baseline of tests/bench_fno3d.py.

What it computes (one model, written down once more so that the package's classes are checked against something that shares no
code with them):

    v = p(x);  v = circular_pad_xy(v, padding)
    for each layer k:   v = act_k( mlp2_k(gelu(mlp1_k(K_k v))) + w_k(v) ),   act_k = gelu, the last one only with last_activation
    v = crop_xy(v, padding);  y = q.mlp2(g(q.mlp1(v))),  g = gelu with last_activation, else nothing;   return y[:, 0]

    K v = irfftn(out, s = mesh),  out zero except the four corner blocks of kept modes, each  einsum(bixyz, ioxyz -> boxyz)
    of the matching block of rfftn(v) with weights1 (low x, low y), weights2 (high x, low y), weights3 (low x, high y),
    weights4 (high x, high y).
"""
import torch
import torch.nn.functional as F


def conv1(x, weight, bias):
    """1x1x1 convolution as a channel einsum: (b, ci, X, Y, T), (co, ci, 1, 1, 1), (co,) -> (b, co, X, Y, T)."""
    out = torch.einsum("oc,bcxyt->boxyt", weight.reshape(weight.shape[0], -1), x)
    return out + bias[None, :, None, None, None] if bias is not None else out


def spectral_conv3d(x, w1, w2, w3, w4):
    b, _, X, Y, T = x.shape
    co, m1, m2, m3 = w1.shape[1:]
    xf = torch.fft.rfftn(x, dim=[-3, -2, -1])
    out = torch.zeros(b, co, X, Y, T // 2 + 1, dtype=xf.dtype, device=x.device)
    mul = lambda blk, w: torch.einsum("bixyz,ioxyz->boxyz", blk, w)
    out[:, :, :m1, :m2, :m3] = mul(xf[:, :, :m1, :m2, :m3], w1)
    out[:, :, -m1:, :m2, :m3] = mul(xf[:, :, -m1:, :m2, :m3], w2)
    out[:, :, :m1, -m2:, :m3] = mul(xf[:, :, :m1, -m2:, :m3], w3)
    out[:, :, -m1:, -m2:, :m3] = mul(xf[:, :, -m1:, -m2:, :m3], w4)
    return torch.fft.irfftn(out, s=(X, Y, T))


def num_layers(sd) -> int:
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("spectral_conv."))


def fno3d_forward(sd, x, padding: int = 0, last_activation: bool = False):
    """``sd``: mapping name -> tensor with the reference's ``state_dict`` keys (on x's device); x (b, input_channel + 3, X, Y, T).
    Returns y (b, X, Y, T)."""
    n = num_layers(sd)
    v = conv1(x, sd["p.weight"], sd["p.bias"])
    if padding:
        v = F.pad(v, [0, 0, padding, padding, padding, padding], mode="circular")
    for k in range(n):
        x1 = spectral_conv3d(v, *[sd[f"spectral_conv.{k}.weights{j}"] for j in (1, 2, 3, 4)])
        x1 = conv1(F.gelu(conv1(x1, sd[f"mlp.{k}.mlp1.weight"], sd[f"mlp.{k}.mlp1.bias"])),
                   sd[f"mlp.{k}.mlp2.weight"], sd[f"mlp.{k}.mlp2.bias"])
        v = x1 + conv1(v, sd[f"w.{k}.weight"], sd[f"w.{k}.bias"])
        if k < n - 1 or last_activation:
            v = F.gelu(v)
    if padding:
        v = v[..., padding:-padding, padding:-padding, :]
    h = conv1(v, sd["q.mlp1.weight"], sd["q.mlp1.bias"])
    if last_activation:
        h = F.gelu(h)
    return conv1(h, sd["q.mlp2.weight"], sd["q.mlp2.bias"]).squeeze(1)


def loss_and_grads(sd, x, target, padding: int = 0, last_activation: bool = False):
    """mean((y - target)^2) and its gradients w.r.t. the input and every entry of ``sd``: (y, grad_x, {name: grad})."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    xl = x.detach().clone().requires_grad_(True)
    y = fno3d_forward(leaves, xl, padding, last_activation)
    loss = ((y - target) ** 2).mean()
    names = list(leaves)
    grads = torch.autograd.grad(loss, [xl] + [leaves[k] for k in names])
    return y.detach(), grads[0], dict(zip(names, grads[1:]))


# the golden cases of tests/golden/make_golden_fno3d.py:
#   name: ((modes1, modes2, modes3), width, input_channel, layers, padding, last_activation, channel_expansion), (b, X, Y, T)
CASES = {
    "tiny": (((4, 3, 3), 8, 5, 4, 0, False, 128), (2, 16, 16, 8)),
    "nb_cover": (((4, 4, 5), 10, 10, 2, 0, False, 128), (2, 8, 8, 10)),
    "pad": (((4, 4, 3), 8, 5, 2, 4, False, 32), (2, 24, 24, 8)),
    "gelu_head": (((3, 3, 2), 20, 10, 2, 0, True, 128), (2, 16, 16, 8)),
    "w16": (((4, 3, 3), 16, 6, 2, 0, False, 64), (1, 16, 32, 12)),
    "w32": (((2, 2, 2), 32, 10, 2, 0, True, 128), (1, 8, 16, 6)),
}
SEED = 11      # torch.manual_seed before the model of a case is built (then the input and the target are drawn)


def ctor_kwargs(case: str) -> dict:
    (modes, width, cin, layers, padding, last, expansion), _ = CASES[case]
    return dict(modes1=modes[0], modes2=modes[1], modes3=modes[2], width=width, input_channel=cin, num_spectral_layers=layers,
                padding=padding, last_activation=last, channel_expansion=expansion)


def case_input(case: str):
    """Input and target of a golden case: smooth fields + the three coordinate channels, from a generator of their own (they do
    not depend on how many numbers the model's initialisation drew)."""
    (_, _, cin, _, _, _, _), (b, X, Y, T) = CASES[case]
    g = torch.Generator().manual_seed(1000 + len(case))
    x = torch.randn(b, cin + 3, X, Y, T, generator=g)
    gx, gy, gt = torch.meshgrid(torch.linspace(0, 1, X), torch.linspace(0, 1, Y), torch.linspace(0, 1, T), indexing="ij")
    x[:, cin:] = torch.stack([gx, gy, gt])[None]
    target = torch.randn(b, X, Y, T, generator=g)
    return x, target
