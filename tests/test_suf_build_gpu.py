"""NeRegSuf(X, y) on the device (RegressionModel.cpp:309-328): X'X by the f64-MFMA syrk in its
XCD-aware tile order (suf_kernel.hip: supertiles of the lower block triangle dealt to the
eight L2s; the supertile's edge depends on how many 64-column tiles there are), X'y, y'y
and the sums -- against numpy at shapes that exercise every edge (1, 2, 4, 8), tile counts
that are no multiple of it, row counts that are no multiple of a panel, and the split over
row slices.  Tolerance: f64 sums in another order.

launch_suf_from_xy has two kernels for X'X: panels by LDS-DMA (xtx_mfma_glds_kernel) when n is
even and X is 16-byte aligned, through registers (xtx_mfma_kernel) otherwise.  An engine's own
upload is aligned, so the parity of n chooses: the odd-n twins of the large shapes send the
register-staged kernel through supertile edges 2, 4, 8 and through split-K; both parities are
run at and below one 32-row step and with trailing row slices that hold no rows; and the two
kernels are required to give the same BYTES (the kernel file's claim) on one X placed at a
16-byte and at an 8-byte boundary."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,p", [(77, 5), (1000, 64), (333, 65), (5000, 130), (2000, 520),
                                 (1500, 1100), (900, 2100), (600, 4200)])
def test_sufficient_statistics_match_numpy(n, p):
    _check_against_numpy(n, p)


# the register-staged kernel (odd n) at supertile edges 8, 4, 2 (p = 4200, 2100, 1100) and with
# split-K over many tiles (p = 520: 45 tiles, 12 slices)
@pytest.mark.parametrize("n,p", [(1501, 1100), (901, 2100), (601, 4200), (2001, 520)])
def test_register_staged_kernel_at_every_supertile_edge(n, p):
    _check_against_numpy(n, p)


# at and below one 32-row step, both parities (so both kernels): a DMA run whose only step is
# partial (n = 2, 30), one whole step (32), a whole and a partial one (34, 33), two (64)
@pytest.mark.parametrize("p", [3, 70])
@pytest.mark.parametrize("n", [1, 2, 30, 31, 32, 33, 34, 64])
def test_steps_at_and_below_one_panel(n, p):
    _check_against_numpy(n, p)


# 17 steps of 32 rows: suf_row_slices gives 16 slices of ceil(17 / 16) = 2 steps, so slices 0-7
# hold 64 rows each, slice 8 the last 18 / 19, and slices 9-15 hold NO rows: their planes must
# come out as zeros for the plane sum
@pytest.mark.parametrize("n,p", [(530, 70), (531, 70)])
def test_trailing_row_slices_without_rows(n, p):
    assert (n + 31) // 32 == 17
    _check_against_numpy(n, p)


def _check_against_numpy(n, p):
    import boom_amd
    rng = np.random.Generator(np.random.PCG64(n + p))
    X = rng.standard_normal((n, p))
    X[:, 0] = 1.0
    y = X[:, : min(p, 4)] @ np.arange(1.0, min(p, 4) + 1.0) + rng.standard_normal(n)
    eng = boom_amd.Engine(2, seed=1)
    eng.build_suf_from_xy(X, y)
    s = eng.get_suf()
    xtx = X.T @ X
    scale = np.sqrt(np.outer(np.diag(xtx), np.diag(xtx)))
    assert np.max(np.abs(s["xtx"] - xtx) / scale) < 1e-13
    assert np.array_equal(s["xtx"], s["xtx"].T)          # mirrored on store: exactly symmetric
    assert np.max(np.abs(s["xty"] - X.T @ y)) < 1e-10 * np.abs(X.T @ y).max()
    assert abs(s["yty"] - y @ y) < 1e-12 * (y @ y)
    assert s["n"] == n
    assert abs(s["ybar"] - y.mean()) < 1e-12 * max(1.0, abs(y.mean()))
    assert np.max(np.abs(s["xbar"] - X.mean(0))) < 1e-12
    # the same call again: bitwise the same statistics (fixed summation order)
    eng.build_suf_from_xy(X, y)
    s2 = eng.get_suf()
    assert np.array_equal(s["xtx"], s2["xtx"]) and np.array_equal(s["xty"], s2["xty"])


def _device_case(n, p):
    import torch
    rng = np.random.Generator(np.random.PCG64(n + p))
    X = rng.standard_normal((n, p))
    X[:, 0] = 1.0
    y = rng.standard_normal(n)
    dev = torch.device("cuda")
    flat = torch.from_numpy(np.asfortranarray(X).ravel(order="F").copy())      # column-major
    aligned = flat.to(dev)
    shifted = torch.empty(n * p + 1, dtype=torch.float64, device=dev)
    shifted[1:].copy_(aligned)
    off = shifted[1:]
    assert aligned.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 8
    yd = torch.from_numpy(y).to(dev)
    torch.cuda.synchronize()
    return X, y, aligned, off, yd, shifted


@pytest.mark.parametrize("n,p", [(1000, 65), (530, 70), (1500, 1100)])
def test_both_kernels_give_the_same_bytes(n, p):
    """n is even, so the aligned copy takes the LDS-DMA kernel; the copy at element 1 of a
    buffer of n p + 1 doubles is 8-byte aligned only and takes the register-staged one: "same
    products in the same order ... bitwise the same X'X" (suf_kernel.hip).  col_reduce_kernel
    does not depend on alignment: X'y, the column means and y'y are the same bytes too."""
    import boom_amd
    X, y, aligned, off, yd, keep = _device_case(n, p)
    out = []
    for ptr in (aligned.data_ptr(), off.data_ptr()):
        eng = boom_amd.Engine(2, seed=1)
        eng.build_suf_from_xy_device(n, p, ptr, yd.data_ptr())
        out.append(eng.get_suf())
    a, b = out
    assert np.array_equal(a["xtx"], b["xtx"])
    assert np.array_equal(a["xty"], b["xty"]) and np.array_equal(a["xbar"], b["xbar"]) and a["yty"] == b["yty"]
    xtx = X.T @ X
    scale = np.sqrt(np.outer(np.diag(xtx), np.diag(xtx)))
    assert np.max(np.abs(b["xtx"] - xtx) / scale) < 1e-13
    assert np.array_equal(b["xtx"], b["xtx"].T)


def test_partial_statistics_of_a_misaligned_shard():
    """suf_partial_device on a shard whose device pointer is 8 but not 16 bytes aligned: the
    block [X'X | X'y | y'y, sum y | column sums] against numpy, and the same bytes as the
    aligned shard gives"""
    import boom_amd
    import torch
    n, p = 530, 70
    X, y, aligned, off, yd, keep = _device_case(n, p)
    eng = boom_amd.Engine(2, seed=1)
    size = eng.suf_block_size(p)
    blocks = []
    for ptr in (aligned.data_ptr(), off.data_ptr()):
        blk = torch.full((size + 8,), -7.0, dtype=torch.float64, device="cuda")
        eng.suf_partial_device(n, p, ptr, yd.data_ptr(), blk.data_ptr())
        torch.cuda.synchronize()
        h = blk.cpu().numpy()
        assert np.all(h[size:] == -7.0)                      # nothing behind the block
        blocks.append(h[:size])
    assert np.array_equal(blocks[0], blocks[1])
    h = blocks[1]
    got = h[:p * p].reshape(p, p)
    xtx = X.T @ X
    scale = np.sqrt(np.outer(np.diag(xtx), np.diag(xtx)))
    assert np.max(np.abs(got - xtx) / scale) < 1e-13
    assert np.array_equal(got, got.T)
    assert np.max(np.abs(h[p * p:p * p + p] - X.T @ y)) < 1e-10 * np.abs(X.T @ y).max()
    assert abs(h[p * p + p] - y @ y) < 1e-12 * (y @ y)
    assert abs(h[p * p + p + 1] - y.sum()) < 1e-12 * max(1.0, np.abs(y).sum())
    assert np.max(np.abs(h[p * p + p + 2:] - X.sum(0))) < 1e-12 * n
