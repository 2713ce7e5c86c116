"""Host-side twin of tests/test_ns2d_n4096_gpu.py (no GPU): which grids the package sends to the fused kernels."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: E402,F401  (puts the repository root on sys.path)


def test_4096_is_a_fused_size_and_8192_is_not():
    from torch_cfd_amd.equations import _is_pow2
    from torch_cfd_amd.mixed_radix import odd_factor_split

    assert _is_pow2(4096)
    assert not _is_pow2(8192)
    assert all(_is_pow2(n) for n in (8, 1024, 2048, 1536, 1280)) and not _is_pow2(4) and not _is_pow2(3072)
    # 4096 has no odd factor: before it was a fused size it fell through to the dense transforms
    assert odd_factor_split(4096) is None


def test_the_size_texts_name_the_new_range():
    """The messages a user reads when a grid is refused say 4096, and the header documents the size and the batch limit."""
    import torch_cfd_amd.equations as eq

    assert "8..4096" in eq.__doc__ and "8..4096" in eq._is_pow2.__doc__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tcfd.h")) as f:
        header = f.read()
    assert "8 ... 4096" in header and "(2^31 - 1) / (n + 18)" in header
