"""Position-embedding resampling without a GPU: the numpy restatement (tests/pos_resample_model.py) against PyTorch's CPU kernels,
its identity cases, and the library's host table (vithip_pos_resample_table) against the restatement, bit for bit.
"""
import numpy as np
import pytest

import pos_resample_model as M
from vit_amd import binding as B

PAIRS = [(14, 24), (14, 16), (14, 28), (14, 32), (2, 3), (14, 7), (24, 14), (8, 5), (3, 2), (1, 4)]
# 4 x the largest |model - F.interpolate| over PAIRS, D = 8, values uniform in [-1, 1] (seed 1000 * g_src + g_dst), measured with
# PyTorch's CPU kernels: 2.36e-6 (bicubic, at 24 -> 14) and 1.08e-6 (antialiased, at 14 -> 24).  PyTorch sums the taps in another
# order (and may fuse), so a few ulp of a 16-term sum of values near 1 are expected; a bound above 1e-5 would mean a wrong formula.
TORCH_BOUND = {"bicubic": 4 * 2.36e-6, "bicubic_aa": 4 * 1.08e-6}


def _pos(g_src: int, g_dst: int, dim: int = 8) -> np.ndarray:
    return np.random.default_rng(1000 * g_src + g_dst).uniform(-1.0, 1.0, (1 + g_src * g_src, dim)).astype(np.float32)


@pytest.mark.parametrize("mode", list(M.MODES))
def test_model_agrees_with_torch_interpolate_on_the_cpu(mode):
    torch = pytest.importorskip("torch")
    worst = 0.0
    for g_src, g_dst in PAIRS:
        pos = _pos(g_src, g_dst)
        got = M.resample(pos, g_dst, mode)
        assert np.array_equal(got[0].view(np.uint32), pos[0].view(np.uint32))  # the class row
        t = torch.from_numpy(pos[1:].reshape(1, g_src, g_src, -1)).permute(0, 3, 1, 2).contiguous()
        ref = torch.nn.functional.interpolate(t, size=(g_dst, g_dst), mode="bicubic", align_corners=False, antialias=mode == "bicubic_aa")
        ref = ref.permute(0, 2, 3, 1).reshape(g_dst * g_dst, -1).numpy()
        err = float(np.abs(got[1:] - ref).max())
        print(f"{mode} {g_src} -> {g_dst}: max |model - torch| = {err:.3e}")
        worst = max(worst, err)
    print(f"{mode}: worst {worst:.3e}, bound {TORCH_BOUND[mode]:.3e}")
    assert worst <= TORCH_BOUND[mode] < 1e-5


@pytest.mark.parametrize("mode", list(M.MODES))
@pytest.mark.parametrize("g", [1, 2, 7, 14])
def test_equal_grids_return_the_bits_of_the_input(mode, g):
    pos = _pos(g, g)
    assert np.array_equal(M.resample(pos, g, mode).view(np.uint32), pos.view(np.uint32))
    for first, w in M.table(mode, g, g):  # weights 0, 1, 0, 0 around the index itself (the antialiased table is cut at the borders)
        assert [float(v) for v in w].count(1.0) == 1 and not any(v for v in w if v != 1.0)


def _assert_table_equal(mode, n_in, n_out):
    want = M.table(mode, n_in, n_out)
    first, count, weights = B.pos_resample_table(mode, n_in, n_out)
    assert weights.shape == (n_out, max(len(w) for _, w in want)), (mode, n_in, n_out)
    for o, (f, w) in enumerate(want):
        assert (int(first[o]), int(count[o])) == (f, len(w)), (mode, n_in, n_out, o)
        assert np.array_equal(weights[o, :len(w)].view(np.uint32), w.view(np.uint32)), (mode, n_in, n_out, o)
        assert not weights[o, len(w):].any()


@pytest.mark.parametrize("mode", list(M.MODES))
def test_host_table_of_the_library_is_the_models_bit_for_bit(mode):
    """Fails where the symbol is absent, and where the host build contracts a product and a sum into an FMA."""
    for n_in in range(1, 41):
        for n_out in range(1, 41):
            _assert_table_equal(mode, n_in, n_out)
    for n_in, n_out in ((14, 24), (14, 32), (24, 14), (64, 16), (256, 255)):
        _assert_table_equal(mode, n_in, n_out)


def test_host_table_refuses_what_it_cannot_build():
    import ctypes as C
    L = B.lib()
    i4, f4 = (C.c_int * 4)(), (C.c_float * 16)()
    for mode, n_in, n_out in ((2, 14, 24), (-1, 14, 24), (0, 0, 4), (0, 257, 4), (1, 4, 0), (1, 4, 257)):
        assert L.vithip_pos_resample_table(mode, n_in, n_out, None, None, None, 0) < 0, (mode, n_in, n_out)
    assert L.vithip_pos_resample_table(0, 4, 4, i4, i4, f4, 3) < 0          # four taps do not fit three
    assert L.vithip_pos_resample_table(0, 4, 4, i4, None, f4, 4) < 0        # some arrays but not all
    assert L.vithip_pos_resample_table(0, 4, 4, None, None, None, 0) == 4   # the sizing call
    assert L.vithip_pos_resample_table(1, 256, 1, None, None, None, 0) == 256
    with pytest.raises(B.VitError):
        B.pos_resample_table("bicubic", 300, 4)
