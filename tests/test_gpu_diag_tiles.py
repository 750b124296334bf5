"""Diagonal tiles of the trailing update cut to the 16 x 16 blocks at or below the diagonal (csrc/gemm_tile.h: gemm_tile_dtv_diag,
taken by syrk_dtv_kernel and syrk_segs_kernel for ti == tj) against the full diagonal tile that TGP_DIAG_FULL=1 selects.

The switch is read once per process, so both settings run in fresh child processes (this file as a script), one child per
setting for all sizes and both solves:
  * the child with TGP_DIAG_FULL=1 writes its packed factors, inverted blocks, `info` and the solves' results to a scratch folder;
  * the child without the switch computes the same, reads the first child's arrays and compares them bit for bit (torch.equal on
    the device for the factors -- 1.4 GB each at the largest size --, numpy.array_equal for the rest).
Each child also factors every matrix a second time with NaN in every 16 x 16 block above the diagonal of every diagonal 128-block
(on top of the tile tests/test_gpu_factor.py poisons) and compares that factor with its un-poisoned one, in the same process.
The tests below assert on what the children report.

That every wave of a diagonal tile computes nine blocks and that the waves' blocks are exactly the blocks j <= i, each once, is
a static_assert next to the tile (diag_deal_cover in gemm_tile.h): a build with a wrong deal does not compile.

Sizes, one per kernel that takes diagonal tiles (see SIZES in tests/test_gpu_factor.py for the schedule at each): Np = 9472 plain
syrk_dtv_kernel bulk launches, 17920 its strips, 18432 and 18688 groups of four with syrk_segs_kernel<4>, <1..3> and the hand-over
to pairs."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_factor as F  # noqa: E402  (family (W), the panel layout and tgp_d_potrf as the factor's own tests use them)

pytestmark = pytest.mark.gpu

PW, TB = F.PW, F.TB
SIZES = [9472, 17920, 18432, 18688]
SOLVES = [18431, 18432]          # tgp_d_gp_solve: y as an augmented row of the last panel / n = Np


def lower_packed(e, P, Np):
    """the packed factor with everything above the diagonal of each panel's 256 x 256 head set to zero: its lower triangle"""
    L = P.clone()
    for p in range(Np // PW):
        off, m = int(e.lib.tgp_panel_off(p, Np)), Np - PW * p
        L[off:off + m * PW].view(m, PW)[:PW].tril_()
    return L


def poison_upper_blocks(e, P, Np):
    """NaN into every 16 x 16 block (i, j), j > i, of every diagonal 128-block of the packed matrix"""
    torch = e.torch
    blk = torch.arange(TB, device=e.dev) // 16
    above = blk[None, :] > blk[:, None]
    for p in range(Np // PW):
        off, m = int(e.lib.tgp_panel_off(p, Np)), Np - PW * p
        head = P[off:off + m * PW].view(m, PW)
        for d in (0, TB):
            head[d:d + TB, d:d + TB].masked_fill_(above, float("nan"))


def child_potrf(e, Np, folder, compare):
    """factor the family (W) matrix of order Np clean and poisoned; write or compare against the other setting's arrays"""
    torch = e.torch
    A = F.family_w(e, Np, Np)
    P = F.pack(e, A)
    Pp = P.clone()
    poison_upper_blocks(e, Pp, Np)
    del A
    info, W = F.potrf(e, P, Np)
    infop, Wp = F.potrf(e, Pp, Np)
    L, Lp = lower_packed(e, P, Np), lower_packed(e, Pp, Np)
    del P, Pp
    rep = {"info": int(info), "info_poisoned": int(infop),
           "finite": bool(torch.isfinite(L).all()) and bool(torch.isfinite(W).all()),
           "poisoned_finite": bool(torch.isfinite(Lp).all()) and bool(torch.isfinite(Wp).all()),
           "poisoned_factor_equal": bool(torch.equal(L, Lp)), "poisoned_blocks_equal": bool(torch.equal(W, Wp))}
    del Lp, Wp
    fl, fw = os.path.join(folder, "L_%d.f64" % Np), os.path.join(folder, "W_%d.f64" % Np)
    if not compare:
        L.cpu().numpy().tofile(fl)
        W.cpu().numpy().tofile(fw)
        with open(os.path.join(folder, "info_%d.json" % Np), "w") as f:
            json.dump(int(info), f)
    else:
        Lo = torch.from_numpy(np.fromfile(fl, dtype=np.float64)).to(e.dev)
        os.remove(fl)
        rep["factor_equal"] = Lo.shape == L.shape and bool(torch.equal(Lo, L))
        rep["factor_differs_at"] = int((Lo != L).sum()) if Lo.shape == L.shape else -1
        del Lo
        rep["blocks_equal"] = bool(np.array_equal(np.fromfile(fw, dtype=np.float64), W.cpu().numpy().ravel()))
        with open(os.path.join(folder, "info_%d.json" % Np)) as f:
            rep["info_equal"] = json.load(f) == int(info)
    return rep


def child_solve(e, n, folder, compare):
    """tgp_d_gp_solve on the star field with the headline kernel: alpha, logdet, y . alpha"""
    import ctypes as C
    from treegp_amd.synthetic import star_field, headline_invlam
    torch = e.torch
    X, y, y_err, _ = star_field(n, 16)
    iL = headline_invlam()
    spec = e.ops.KernelSpec(e._lib.TGP_ARBF, amp=1.0, a=iL[0, 0], b=iL[0, 1], c=iL[1, 1])
    prob = e.ops.ResidentProblem(X, y - y.mean(), y_err, ctx=e.ctx)
    try:
        alpha = torch.empty(n, dtype=torch.float64, device=e.dev)
        logdet, ydota = C.c_double(0.0), C.c_double(0.0)
        torch.cuda.synchronize()
        rc = e.lib.tgp_d_gp_solve(e.ctx, C.byref(spec.to_c()), prob.d_X, n, prob.d_y, prob.d_e, F._vp(alpha), C.byref(logdet),
                                  C.byref(ydota), None)
        e._lib.check(e.ctx, rc, "tgp_d_gp_solve")
    finally:
        prob.close()
    a = alpha.cpu().numpy()
    res = np.concatenate([a, [logdet.value, ydota.value]])
    rep = {"rc": int(rc), "finite": bool(np.isfinite(res).all())}
    fa = os.path.join(folder, "solve_%d.f64" % n)
    if not compare:
        res.tofile(fa)
    else:
        other = np.fromfile(fa, dtype=np.float64)
        rep["alpha_equal"] = bool(np.array_equal(other[:-2], a))
        rep["logdet_equal"] = bool(other[-2] == logdet.value)
        rep["ydota_equal"] = bool(other[-1] == ydota.value)
    return rep


def child_main(folder, compare):
    e = F._env()
    out = {"diag_full": os.environ.get("TGP_DIAG_FULL", ""), "potrf": {}, "solve": {}}
    for Np in SIZES:
        out["potrf"][str(Np)] = child_potrf(e, Np, folder, compare)
        e.torch.cuda.empty_cache()
    for n in SOLVES:
        out["solve"][str(n)] = child_solve(e, n, folder, compare)
    with open(os.path.join(folder, "report_%s.json" % ("half" if compare else "full")), "w") as f:
        json.dump(out, f)
    print("DIAG CHILD OK")


@pytest.fixture(scope="module")
def reports():
    """(report of the child with TGP_DIAG_FULL=1, report of the child without it, which compared itself against the first)"""
    here = os.path.abspath(__file__)
    with tempfile.TemporaryDirectory(prefix="tgp_diag_") as folder:
        out = []
        for compare in (False, True):
            env = dict(os.environ)
            env.pop("TGP_DIAG_FULL", None)
            if not compare:
                env["TGP_DIAG_FULL"] = "1"
            r = subprocess.run([sys.executable, here, folder, "compare" if compare else "write"], env=env, capture_output=True,
                               text=True, timeout=600)
            print(r.stdout[-2000:])
            assert r.returncode == 0 and "DIAG CHILD OK" in r.stdout, (compare, r.stdout[-1500:], r.stderr[-3000:])
            with open(os.path.join(folder, "report_%s.json" % ("half" if compare else "full"))) as f:
                out.append(json.load(f))
    assert out[0]["diag_full"] == "1" and out[1]["diag_full"] == ""
    return out


@pytest.mark.parametrize("Np", SIZES)
def test_same_bits_as_the_full_diagonal_tile(reports, Np):
    """tgp_d_potrf on (W): the packed factor's lower triangle, the inverted blocks W and `info` are equal bit for bit between the
    full diagonal tile (TGP_DIAG_FULL=1) and the nine-blocks-per-wave one."""
    full, half = reports[0]["potrf"][str(Np)], reports[1]["potrf"][str(Np)]
    assert full["info"] == 0 and half["info"] == 0, (full, half)
    assert full["finite"] and half["finite"], (full, half)
    assert half["info_equal"], (full, half)
    assert half["factor_equal"], "factor differs at %d entries" % half["factor_differs_at"]
    assert half["blocks_equal"], "inverted blocks differ"


@pytest.mark.parametrize("Np", SIZES)
@pytest.mark.parametrize("setting", ["full", "half"])
def test_nothing_reads_the_blocks_above_the_diagonal(reports, Np, setting):
    """NaN in every 16 x 16 block above the diagonal of every diagonal 128-block of the input (which the cut tile neither reads nor
    writes), and in the tile tests/test_gpu_factor.py poisons: the factor is finite and has the bits of the un-poisoned run, with
    and without the switch."""
    rep = reports[0 if setting == "full" else 1]["potrf"][str(Np)]
    assert rep["info_poisoned"] == 0, rep
    assert rep["poisoned_finite"], rep
    assert rep["poisoned_factor_equal"] and rep["poisoned_blocks_equal"], rep


@pytest.mark.parametrize("n", SOLVES)
def test_one_solve_through_the_public_entry(reports, n):
    """tgp_d_gp_solve at n = 18431 (y rides as an augmented row) and n = 18432: alpha, logdet and y . alpha equal bit for bit
    between the two settings of the switch."""
    full, half = reports[0]["solve"][str(n)], reports[1]["solve"][str(n)]
    assert full["rc"] == 0 and half["rc"] == 0, (full, half)
    assert full["finite"] and half["finite"], (full, half)
    assert half["alpha_equal"] and half["logdet_equal"] and half["ydota_equal"], half


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    child_main(sys.argv[1], sys.argv[2] == "compare")
