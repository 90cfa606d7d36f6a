"""Checks of the Q2n index (include/ddif.h ddif_q2n, ddif.runtime.q2n / q_avg), shared by tests/test_q2n_emu.py (host-emulated build, CPU tensors) and
tests/test_q2n_gpu.py (the gfx950 library).  The fixtures (tests/golden/q2n_*.npz, tools/make_golden.py --only q2n) hold integer-valued images, the block
values of a composition of the reference's own norm_blocco / onion_mult / onion_mult2D in fp64, and `sens`: how far each block's value moves when the
composition sums its pixels in another order.

Tolerance of the value checks: both sides are fp64 and differ in operation order and contraction only, so per block |Q - golden| <= max(1e-13, 100 sens):
the golden's own order sensitivity (a few 1e-15 on these blocks, 1.6e-14 at most) with a margin of 100, floored at 1e-13.  Every figure is printed before
it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import golden_cases_q2n as gq
from ddif import runtime
from ddif.runtime import DdifError


@functools.lru_cache(maxsize=None)
def fixture(name):
    return gq.load(name)


def _dev_tensor(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _run(fx, pair, dev, scale=1.0):
    _, _, _, _, block, shift, _, _ = (int(v) for v in fx["geometry"])
    q, m = runtime.q2n(_dev_tensor(fx["gt"], dev), _dev_tensor(fx[f"pred_{pair}"], dev), scale, block, shift, return_map=True)
    assert q.dtype == torch.float64 and m.dtype == torch.float64 and tuple(m.shape) == fx[f"map_{pair}"].shape and tuple(q.shape) == (fx["gt"].shape[0],)
    return q.cpu().numpy(), m.cpu().numpy()


def _block_check(name, pair, got, want, sens):
    tol = np.maximum(1e-13, 100.0 * sens)
    err = np.abs(got - want)
    print(f"{name}/{pair}: max|Q - golden| = {err.max():.3e} (tolerance >= {tol.min():.1e}, order sensitivity <= {sens.max():.2e})")
    assert np.isfinite(got).all() and (err <= tol).all(), (name, pair, float(err.max()))
    return float(err.max())


def run_fixture(case, dev):
    """test 1: every block of every image pair of a regular case against the golden"""
    fx = fixture(case[0])
    worst = 0.0
    for pair in gq.PAIRS:
        q, m = _run(fx, pair, dev)
        worst = max(worst, _block_check(case[0], pair, m, fx[f"map_{pair}"], fx[f"sens_{pair}"]))
        want = fx[f"map_{pair}"].mean(axis=(1, 2))  # the image value is the mean of the blocks: no worse than the worst block
        tol = max(1e-13, 100.0 * float(fx[f"sens_{pair}"].max()))
        print(f"{case[0]}/{pair}: Q2n = {q}, |Q2n - golden| = {np.abs(q - want).max():.3e}")
        assert (np.abs(q - want) <= tol).all()
        assert (m >= 0).all() and (m <= 1 + 1e-12).all()
    return worst


def run_identical(case, dev):
    """test 2: two identical images score 1 in every block (the reference's `q2n` gives 0.87 .. 2.06 there)"""
    fx = fixture(case[0])
    q, m = _run(fx, "identical", dev)
    print(f"{case[0]}: identical images, max|Q - 1| = {np.abs(m - 1).max():.3e} per block, {np.abs(q - 1).max():.3e} per image")
    assert np.abs(m - 1).max() <= 4e-15 and np.abs(q - 1).max() <= 4e-15


def run_degenerate(dev):
    """test 3: the three constructed blocks of the degenerate fixture, and its regular fourth"""
    fx = fixture(gq.DEGENERATE[0])
    _, m = _run(fx, "noise", dev)
    want, sens = fx["map_noise"], fx["sens_noise"]
    assert fx["T3_noise"][0, 0, 0] == 0 and (fx["t_noise"][0, 0, 1, 2] == 1e-8) and (fx["s_noise"][0, 1, 0] == 0).all()  # the fixture is what it says
    print(f"degenerate: T3 == 0 block Q = {m[0, 0, 0]!r}")
    assert abs(m[0, 0, 0] - 1) <= 4e-15
    for label, (j, i) in (("constant gt band", (0, 1)), ("all-zero gt", (1, 0))):
        got, ref, sn = m[0, j, i], want[0, j, i], sens[0, j, i]
        compared = sn < 1e-3 * ref
        print(f"degenerate: {label}: Q = {got!r}, golden {ref!r}, order sensitivity {sn:.2e}, compared: {bool(compared)}")
        assert np.isfinite(got) and got >= 0
        if compared:
            assert abs(got - ref) <= 100.0 * sn
    _block_check(gq.DEGENERATE[0], "regular block", m[:, 1:, 1:], want[:, 1:, 1:], sens[:, 1:, 1:])


def run_rounding(dev):
    """test 4: the quantisation rounds (the MATLAB original's uint16()), it does not truncate (the Python port's astype): counts / 2047 in fp32 times
    scale = 2047 gives the counts back, bit for bit.  The fp32 product of fl(i / 2047) and 2047 is i itself, so truncation shows only on normalised values
    that sit just below i / 2047 -- what 1023 / 2047 * 2047 = 1022.9999999999999 is in Python doubles: every seventh value here is moved down by one
    fp32 ulp, where flooring the product loses a count and rounding does not."""
    fx = fixture("q2n_c4_64")
    gt, pred = (fx["gt"] % 2048).astype(np.float32), (fx["pred_noise"] % 2048).astype(np.float32)
    gt[0, 0, 0, :4] = (1023, 2047, 1, 341)
    gn, pn = gt / np.float32(2047), pred / np.float32(2047)
    for a in (gn, pn):
        a.reshape(-1)[::7] = np.nextafter(a.reshape(-1)[::7], np.float32(0))
    lost = int((np.floor(gn * np.float32(2047)) != gt).sum() + (np.floor(pn * np.float32(2047)) != pred).sum())
    print(f"rounding: truncation would lose a count on {lost} of {gt.size + pred.size} values")
    assert lost > 0 and (np.rint(gn * np.float32(2047)) == gt).all() and (np.rint(pn * np.float32(2047)) == pred).all()
    q1, m1 = runtime.q2n(_dev_tensor(gt, dev), _dev_tensor(pred, dev), 1.0, 32, 32, return_map=True)
    q2, m2 = runtime.q2n(_dev_tensor(gn, dev), _dev_tensor(pn, dev), 2047.0, 32, 32, return_map=True)
    assert torch.equal(m1, m2) and torch.equal(q1, q2)


def run_batch_and_repeat(dev):
    """test 5: a batch of two is bit-equal to its images run alone, and to itself run again"""
    fx = fixture("q2n_c4_48_b2")
    gt, pred = _dev_tensor(fx["gt"], dev), _dev_tensor(fx["pred_noise"], dev)
    q, m = runtime.q2n(gt, pred, 1.0, 32, 32, return_map=True)
    q_again, m_again = runtime.q2n(gt, pred, 1.0, 32, 32, return_map=True)
    assert torch.equal(q, q_again) and torch.equal(m, m_again)
    assert torch.equal(runtime.q2n(gt, pred, 1.0, 32, 32), q)  # without the map: the same values
    for b in range(2):
        qb, mb = runtime.q2n(gt[b:b + 1], pred[b:b + 1], 1.0, 32, 32, return_map=True)
        assert torch.equal(qb, q[b:b + 1]) and torch.equal(mb, m[b:b + 1])
    assert not torch.equal(m[0], m[1])


def run_q_avg(dev):
    """test 6: q_avg = the mean over the bands of the single-band index"""
    fx = fixture("q2n_c4_48_b2")
    gt, pred = _dev_tensor(fx["gt"], dev), _dev_tensor(fx["pred_noise"], dev)
    got = runtime.q_avg(gt, pred, 1.0, 32, 16)
    bands = [runtime.q2n(gt[:, c:c + 1].contiguous(), pred[:, c:c + 1].contiguous(), 1.0, 32, 16) for c in range(gt.shape[1])]
    want = torch.stack(bands, dim=1).mean(dim=1)
    print(f"q_avg = {got.cpu().numpy()}")
    assert got.dtype == torch.float64 and torch.equal(got, want)
    assert float(got.min()) > 0 and float(got.max()) < 1


def run_validation(dev):
    """test 7: every refusal of the C ABI raises DdifError and names the argument"""
    lib = runtime.get_lib()
    gt, pred = torch.rand(1, 4, 8, 8).to(dev), torch.rand(1, 4, 8, 8).to(dev)
    q = torch.empty(1, dtype=torch.float64, device=gt.device)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def raw(g=gt, p=pred, B=1, Cc=4, H=8, W=8, scale=1.0, block=4, shift=4, out=q):
        lib.check(lib.dll.ddif_q2n(vp(g), vp(p), B, Cc, H, W, scale, block, shift, None, vp(out), None), "ddif_q2n")

    raw()  # the baseline call is accepted
    for kw, names in ((dict(g=None), r"\bgt\b"), (dict(p=None), r"\bpred\b"), (dict(out=None), r"\bq_out\b"), (dict(Cc=0), r"\bC=0\b"), (dict(Cc=9), r"\bC=9\b"),
                      (dict(block=1), r"\bblock=1\b"), (dict(block=65, shift=8), r"\bblock=65\b"), (dict(shift=0), r"\bshift=0\b"),
                      (dict(shift=5), r"\bshift=5\b"), (dict(H=0), r"\bH=0\b"), (dict(W=0), r"\bW=0\b"), (dict(B=0), r"\bB=0\b"),
                      (dict(scale=0.0), r"\bscale=0\b"), (dict(scale=-1.0), r"\bscale=-1\b"), (dict(scale=float("nan")), r"\bscale=-?nan\b"),
                      (dict(scale=float("inf")), r"\bscale=inf\b")):
        with pytest.raises(DdifError, match=names):
            raw(**kw)
    # the same refusals reach the caller of the Python binding; tensors are validated like runtime.metrics does
    big = torch.rand(1, 9, 8, 8).to(dev)
    with pytest.raises(DdifError, match=r"\bC=9\b"):
        runtime.q2n(big, big)
    with pytest.raises(DdifError, match=r"\bblock=65\b"):
        runtime.q2n(gt, pred, block=65)
    with pytest.raises(DdifError, match=r"\bshift=0\b"):
        runtime.q2n(gt, pred, shift=0)
    with pytest.raises(DdifError, match=r"\bscale=0\b"):
        runtime.q2n(gt, pred, scale=0.0)
    with pytest.raises(DdifError, match="pred"):
        runtime.q2n(gt, pred[:, :3])
    with pytest.raises(DdifError, match="float32"):
        runtime.q2n(gt.double(), pred.double())
    with pytest.raises(DdifError, match="gt"):
        runtime.q2n(gt[0], pred[0])
    with pytest.raises(DdifError, match="pred"):
        runtime.q_avg(gt, pred[:, :3])
