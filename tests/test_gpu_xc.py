"""The five kernels of the exchange-correlation chain on the MI355X against the extended-precision references of
tests/xc_reference.py: nbx_xc_functional (50-digit sympy / mpmath energy densities and symbolic derivatives),
nbx_xc_rho, nbx_xc_vmat, nbx_eval_ao and nbx_becke_share (numpy.longdouble), then the whole chain on the H atom
(alpha density one orbital, beta density identically zero: the fully polarised configuration).

Bounds.  The functional: 5e-11 relative per entry, 1e-12 on E_xc and the electron count, entries whose exact value
is below 1e-150 measured against 1e-150 (a condition: LYP's exponential underflows in float64 where nothing
physical lives).  The contractions and eval_ao: the rounding bound of a float64 evaluation, per entry, derived in
the docstrings of the reference functions.  Becke shares: rtol 1e-9, atol 1e-13, the project's figures.

Reference cost: 150 points per regime x 10 regimes x 4 functionals = 6000 points at 50 digits (15 s), 1800 more
for the H atom; the longdouble contractions take about as long again.
"""

from types import SimpleNamespace

import numpy as np
import pytest

import xc_reference as xr

pytestmark = pytest.mark.gpu

FLOOR = 1e-14


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


# ------------------------------------------------------------------------------------------------ nbx_xc_functional
def _kernel_functional(be, name, rho, grad, w):
    from nbed_amd import _nbx

    vr, vec, sums = be.xc_functional(_nbx.XC_CODES[name], be.asarray(rho), be.asarray(grad), be.asarray(w), FLOOR)
    sums = be.to_host(sums)
    return be.to_host(vr), be.to_host(vec), float(sums[0]), float(sums[1])


def _all_regimes(name):
    """Every regime in one launch: 1500 points, six blocks, the last one partial."""
    import mpmath as mp

    ins = [xr.regime_inputs(r, FLOOR) for r in xr.REGIMES]
    refs = [xr.regime_reference(name, r, FLOOR) for r in xr.REGIMES]
    with mp.workdps(xr.DPS):
        exc, nelec = sum(r[2] for r in refs), sum(r[3] for r in refs)
    ref = (np.concatenate([r[0] for r in refs], axis=1), np.concatenate([r[1] for r in refs], axis=2), exc, nelec,
           np.concatenate([r[4] for r in refs]))
    return tuple(np.concatenate([i[k] for i in ins], axis=-1) for k in range(3)), ref


@pytest.mark.parametrize("regime", xr.REGIMES + ("all",))
@pytest.mark.parametrize("name", xr.FUNCTIONALS)
def test_functional_kernel_against_the_50_digit_reference(be, name, regime):
    from nbed_amd import xc

    assert xc.XCProvider.RHO_FLOOR == FLOOR
    if regime == "all":
        (rho, grad, w), ref = _all_regimes(name)
        assert rho.shape[1] > 256 and rho.shape[1] % 256
    else:
        rho, grad, w = xr.regime_inputs(regime, FLOOR)
        ref = xr.regime_reference(name, regime, FLOOR)
        assert 64 <= rho.shape[1] and rho.shape[1] % 256
    xr.check_functional(f"kernel {name} {regime}", _kernel_functional(be, name, rho, grad, w), ref)


@pytest.mark.parametrize("regime,index", [("existing", 0), ("polarised_beta_empty", 0), ("polarised_alpha_empty", 149),
                                          ("at_floor", 0), ("at_floor", 1)])
@pytest.mark.parametrize("name", xr.FUNCTIONALS)
def test_functional_kernel_on_a_grid_of_one_point(be, name, regime, index):
    rho, grad, w = xr.regime_inputs(regime, FLOOR)
    rho, grad, w = rho[:, index:index + 1], grad[:, :, index:index + 1], w[index:index + 1]
    ref = xr.functional_reference(name, rho, grad, w, FLOOR)
    if regime == "at_floor":
        assert bool(ref[4][0]) == bool(index)  # exactly on the floor: dropped; one ulp above: kept
    xr.check_functional(f"kernel {name} {regime}[{index}]", _kernel_functional(be, name, rho, grad, w), ref)


# ------------------------------------------------------------------------------------------------ nbx_xc_rho
def _scaled_aos(rng, g, nao):
    """AO rows whose size varies over eight orders of magnitude from grid point to grid point; the first and the last
    point are full size, so that a lost edge of the grid is not hidden behind larger neighbours."""
    scale = 10 ** rng.uniform(-8, 0, g)
    scale[0] = scale[-1] = 1.0
    ao = rng.normal(size=(g, nao)) * scale[:, None]
    dao = rng.normal(size=(3, g, nao)) * scale[None, :, None]
    return ao, dao


RHO_SMALL = [(g, n) for n in (1, 3, 4, 5, 15, 16, 17) for g in (1, 15, 16, 17, 63, 64, 65, 257)]
RHO_LARGE = [(g, n) for n in (156, 157, 160, 161, 164, 165, 637, 640) for g in (1, 17, 65, 257)]


@pytest.mark.parametrize("g,nao", RHO_SMALL + RHO_LARGE)
def test_rho_kernel_within_the_rounding_bound_of_every_entry(be, g, nao):
    """Both register variants (A fragments kept for (nao + 3 & ~3) <= 160: 157..160 on one side, 161..164 on the
    other), up to the LDS limit of 640 functions, partial 16-point waves and partial 64-point workgroups."""
    rng = np.random.default_rng(100000 * g + nao)
    ao, dao = _scaled_aos(rng, g, nao)
    dm = rng.normal(size=(2, nao, nao))
    dm = 0.5 * (dm + dm.transpose(0, 2, 1))
    rho, grad = be.xc_rho(be.asarray(ao), be.asarray(dao), be.asarray(dm))
    want_rho, want_grad, b_rho, b_grad = xr.rho_reference(ao, dao, dm)
    e_rho = np.abs(be.to_host(rho).astype(xr.LD) - want_rho).astype(np.float64)
    e_grad = np.abs(be.to_host(grad).astype(xr.LD) - want_grad).astype(np.float64)
    print(f"XCRHO g {g} nao {nao} worst err/bound rho {np.max(e_rho / b_rho):.3f} grad {np.max(e_grad / b_grad):.3f}")
    assert np.all(e_rho <= b_rho) and np.all(e_grad <= b_grad)  # (NaN fails)


def test_rho_kernel_refuses_what_does_not_fit_the_lds(be):
    from nbed_amd import _nbx

    rng = np.random.default_rng(641)
    ao, dao = _scaled_aos(rng, 3, 641)
    with pytest.raises(_nbx.NbxError) as err:
        be.xc_rho(be.asarray(ao), be.asarray(dao), be.asarray(np.zeros((2, 641, 641))))
    assert err.value.code == _nbx.NBX_E_UNSUPPORTED and "640" in str(err.value)


# ------------------------------------------------------------------------------------------------ nbx_xc_vmat
def vmat_bt(nao):
    """csrc/xc.hip's rule: tiles per block side -- the least padded 16 bt grid over nao, the larger bt on a tie."""
    best, best_pad = 1, None
    for bt in range(1, 6):
        pad = -(-nao // (16 * bt)) * 16 * bt
        if best_pad is None or pad <= best_pad:
            best, best_pad = bt, pad
    return best


def vmat_chunk(npts, nao):
    nblk = -(-nao // (16 * vmat_bt(nao)))
    chunk = 2048
    while chunk > 256 and -(-npts // chunk) * nblk * nblk * 2 < 1024:
        chunk >>= 1
    return chunk


VMAT_NAO = (16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 148)
VMAT_G = (1, 15, 17, 255, 257, 2047, 2049, 4097)
VMAT_CASES = sorted({(g, n) for n in VMAT_NAO for g in (1, 17, 257, 2049)} | {(g, n) for n in (16, 33, 148) for g in VMAT_G})
VMAT_CHUNK_CASES = [(8200, 176, 2048), (4097, 176, 1024), (2049, 176, 512), (257, 176, 256)]


def test_vmat_cases_cover_every_block_and_chunk_size():
    assert [vmat_bt(n) for n in VMAT_NAO] == [1, 2, 2, 3, 3, 4, 4, 5, 5, 3, 3, 1, 5]
    assert all(vmat_chunk(g, n) == c for g, n, c in VMAT_CHUNK_CASES) and vmat_bt(176) == 1
    assert {c for _, _, c in VMAT_CHUNK_CASES} == {2048, 1024, 512, 256}


@pytest.mark.parametrize("g,nao", VMAT_CASES + [(g, n) for g, n, _ in VMAT_CHUNK_CASES])
def test_vmat_kernel_within_the_rounding_bound_of_every_entry(be, g, nao):
    rng = np.random.default_rng(100000 * g + nao)
    ao, dao = _scaled_aos(rng, g, nao)
    vr, vec = rng.normal(size=(2, g)), rng.normal(size=(2, 3, g))
    nchunk = -(-g // vmat_chunk(g, nao))  # the workspace the library asks for tells which chunk size it chose
    assert int(be.lib.nbx_xc_vmat_worksize(g, nao)) == (nchunk * 2 * nao * nao * 8 + 255) // 256 * 256
    dev = [be.asarray(x) for x in (ao, dao, vr, vec)]
    got = be.to_host(be.xc_vmat(*dev))
    want, bound = xr.vmat_reference(ao, dao, vr, vec)
    err = np.abs(got.astype(xr.LD) - want).astype(np.float64)
    print(f"XCVMAT g {g} nao {nao} bt {vmat_bt(nao)} chunk {vmat_chunk(g, nao)} worst err/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    np.testing.assert_array_equal(got, got.transpose(0, 2, 1))
    np.testing.assert_array_equal(be.to_host(be.xc_vmat(*dev)), got)  # run to run: the same bits


# ------------------------------------------------------------------------------------------------ nbx_eval_ao
_CART = {0: [(0, 0, 0)], 1: [(1, 0, 0), (0, 1, 0), (0, 0, 1)],
         2: [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2)],
         3: [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]}
CENTRES = np.array([[0.0, 0.0, 0.25], [0.3, 1.4, -0.9]])


def _hand_built_shells(nprim_s=24):
    """s (``nprim_s`` primitives), p, d and f shells on two centres; every exponent >= 0.5."""
    rng = np.random.default_rng(24)
    shells = []
    for centre in CENTRES:
        for ang, nk in ((0, nprim_s), (1, 3), (2, 2), (3, 1), (0, 1)):
            exps = 0.5 * 10 ** rng.uniform(0, 4 if ang == 0 else 1.5, nk)
            coefs = rng.normal(size=(len(_CART[ang]), nk))
            shells.append((centre, exps, coefs, _CART[ang]))
    return shells


def _table(be, shells):
    """The device table of HipBackend.ao_table from plain shell data."""
    ns = [SimpleNamespace(centre=c, exps=e, coefs=k, cart=lmn) for c, e, k, lmn in shells]
    ao0 = np.cumsum([0] + [len(s.cart) for s in ns])
    return be.ao_table(SimpleNamespace(shells=ns, shell_ao0=list(ao0[:-1]), nao_cart=int(ao0[-1])))


def _points(centres, n):
    """On each nucleus, 1e-8 bohr from each, 40 bohr away, then points scattered about the molecule."""
    rng = np.random.default_rng(n)
    special = [c for c in centres] + [c + np.array([6e-9, -8e-9, 0.0]) for c in centres] + [centres[0] + [0.0, 40.0, 30.0]]
    pts = np.concatenate([np.array(special), centres[rng.integers(len(centres), size=n)] + rng.normal(scale=1.5, size=(n, 3))])
    return np.ascontiguousarray(pts[:n]), len(centres), 2 * len(centres)


def _check_ao(be, shells, pts, label):
    table = _table(be, shells)
    ao, dao = be.eval_ao(be.asarray(pts), table, deriv=True)
    ao, dao = be.to_host(ao), be.to_host(dao)
    want, dwant, bound, dbound = xr.ao_reference(shells, pts)
    err = np.abs(ao.astype(xr.LD) - want).astype(np.float64)
    derr = np.abs(dao.astype(xr.LD) - dwant).astype(np.float64)
    print(f"XCAO {label} g {pts.shape[0]} worst err/bound ao {np.max(err / bound):.3f} dao {np.max(derr / dbound):.3f}")
    assert np.all(err <= bound) and np.all(derr <= dbound)
    only, none = be.eval_ao(be.asarray(pts), table, deriv=False)
    assert none is None
    np.testing.assert_array_equal(be.to_host(only), ao)  # values alone: the same bits
    return ao, dao


@pytest.mark.parametrize("g", [1, 255, 256, 257])
def test_eval_ao_hand_built_shells_within_the_rounding_bound(be, g):
    shells = _hand_built_shells()
    assert max(len(s[1]) for s in shells) == 24 and {max(map(sum, s[3])) for s in shells} == {0, 1, 2, 3}
    pts, on_nucleus, far = _points(CENTRES, g)
    ao, dao = _check_ao(be, shells, pts, "hand-built")
    assert np.abs(ao[0]).max() > 0.0  # the point on the first nucleus sees its s shells
    if g > far:
        assert np.linalg.norm(pts[far] - CENTRES, axis=1).min() >= 40.0
        assert np.all(ao[far] == 0.0) and np.all(dao[:, far] == 0.0)  # exp(-a r^2) <= exp(-800): exact zeros, no NaN
        assert np.abs(ao[on_nucleus:far]).max() > 0.0


def test_eval_ao_refuses_a_shell_of_25_primitives(be):
    from nbed_amd import _nbx

    shells = _hand_built_shells(nprim_s=25)
    with pytest.raises(_nbx.NbxError) as err:
        be.eval_ao(be.asarray(_points(CENTRES, 4)[0]), _table(be, shells))
    assert err.value.code == _nbx.NBX_E_UNSUPPORTED and "24" in str(err.value)


def test_eval_ao_ccpvtz_water_within_the_rounding_bound(be):
    from nbed_amd import integrals

    water = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
    atoms = integrals.parse_geometry(water, "angstrom")
    bs = integrals.Basis(atoms, "cc-pvtz")
    shells = [(sh.centre, sh.exps, sh.coefs, [tuple(lmn) for lmn in sh.cart]) for sh in bs.shells]
    assert {max(map(sum, s[3])) for s in shells} == {0, 1, 2, 3}
    centres = np.array([pos for _, pos in atoms])
    pts, _, _ = _points(centres, 600)
    _check_ao(be, shells, pts, "cc-pvtz water")


# ------------------------------------------------------------------------------------------------ nbx_becke_share
def _share(be, pts, centres, aij, inv, owner):
    return be.to_host(be.becke_share(be.asarray(pts), be.asarray(centres), be.asarray(aij), be.asarray(inv), owner))


def _cluster(natm, seed, box=6.0):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-box, box, size=(natm, 3))
    chi = rng.uniform(0.5, 2.0, size=natm)
    chi = chi[:, None] / chi[None, :]
    uab = (chi - 1.0) / (chi + 1.0)
    aij = np.clip(uab / (uab * uab - 1.0), -0.5, 0.5)
    np.fill_diagonal(aij, 0.0)
    dist = np.linalg.norm(centres[:, None] - centres[None], axis=-1)
    return centres, aij, 1.0 / (dist + np.eye(natm))


def test_becke_share_exact_cases(be):
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(300, 3))
    one = _share(be, pts, np.array([[0.1, 0.2, 0.3]]), np.zeros((1, 1)), np.ones((1, 1)), 0)
    np.testing.assert_array_equal(one, np.ones(300))  # a single atom owns everything
    centres = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    inv = np.array([[1.0, 0.5], [0.5, 1.0]])
    plane = np.concatenate([np.zeros((300, 1)), rng.normal(scale=3.0, size=(300, 2))], axis=1)
    for owner in (0, 1):  # equal sizes, equal distances: mu = 0, each cell is 1/2
        np.testing.assert_array_equal(_share(be, plane, centres, np.zeros((2, 2)), inv, owner), np.full(300, 0.5))
    on = np.ascontiguousarray(centres)
    np.testing.assert_array_equal(_share(be, on, centres, np.zeros((2, 2)), inv, 0), [1.0, 0.0])  # mu = -1, +1 exactly
    np.testing.assert_array_equal(_share(be, on, centres, np.zeros((2, 2)), inv, 1), [0.0, 1.0])


@pytest.mark.parametrize("natm", [2, 95, 96, 97])
def test_becke_share_against_longdouble(be, natm):
    """Either side of the size at which the atom-pair tables leave the LDS; first, middle and last owner; points
    scattered through the cluster, on two nuclei and just off one."""
    centres, aij, inv = _cluster(natm, natm)
    rng = np.random.default_rng(natm + 1)
    pts = np.concatenate([rng.uniform(-7, 7, size=(297, 3)), centres[:1], centres[-1:], centres[:1] + 1e-8])
    for owner in (0, natm // 2, natm - 1):
        got = _share(be, pts, centres, aij, inv, owner)
        want = xr.becke_reference(pts, centres, aij, inv, owner).astype(np.float64)
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-13)


def test_becke_share_far_from_a_large_cluster_is_finite(be):
    centres, aij, inv = _cluster(100, 7)
    far = np.array([[50.0, 0.0, 0.0], [0.0, -50.0, 0.0], [30.0, 30.0, 26.0], [-29.0, 29.0, -29.0]])
    far = far * (50.0 / np.linalg.norm(far, axis=1))[:, None] + centres.mean(axis=0)
    total = np.zeros(len(far))
    for owner in range(100):
        got = _share(be, far, centres, aij, inv, owner)
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0) and np.all(got <= 1.0), (owner, got)
        want = xr.becke_reference(far, centres, aij, inv, owner).astype(np.float64)
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-13)
        total += got
    np.testing.assert_allclose(total, 1.0, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the whole chain
@pytest.mark.parametrize("name", ["b3lyp", "lda,vwn"])
def test_h_atom_open_shell_chain(be, name):
    """H / 6-31G, one alpha electron, no beta electron, on a 24 x 6 x 12 product grid (1728 points): XCProvider on
    the device (eval_ao, xc_rho, xc_functional, xc_vmat) against XCProvider on the host and against the references
    chained on the same points -- E_xc summed at 50 digits, v_xc of both spins contracted in longdouble from the
    50-digit vr / vec.  E_xc: 1e-12 relative to the host (the functional's bound on the sum) and 1e-11 to the
    reference, which takes rho from the exact AOs (rho carries (2 nao + 4) u and E_xc goes as rho^(4/3)); v_xc: 1e-10
    of the largest entry of each spin -- twice the functional's 5e-11 per entry, every entry being a sum over the grid
    of terms of mixed sign."""
    from nbed_amd import integrals, xc

    atoms = integrals.parse_geometry("1\n\nH 0.0 0.0 0.0", "angstrom")
    bs = integrals.Basis(atoms, "6-31g")
    s = integrals.molecule_integrals("1\n\nH 0.0 0.0 0.0", "6-31g")["S"]
    c = np.array([0.45, 0.65])
    c = c / np.sqrt(c @ s @ c)
    dm = np.stack([np.outer(c, c), np.zeros((2, 2))])
    dev = xc.XCProvider(atoms, bs, name, n_rad=32, n_theta=6, device=be.device)
    host = xc.XCProvider(atoms, bs, name, n_rad=32, n_theta=6, device="cpu")
    np.testing.assert_array_equal(dev.points, host.points)
    npts = dev.points.shape[0]
    assert 1000 < npts < 2500 and bs.pure_cartesian
    e_dev, v_dev = dev(dm)
    e_host, v_host = host(dm)
    shells = [(sh.centre, sh.exps, sh.coefs, [tuple(lmn) for lmn in sh.cart]) for sh in bs.shells]
    ao, dao, _, _ = xr.ao_reference(shells, dev.points)
    dml = np.asarray(dm, dtype=xr.LD)
    cmat = np.stack([ao @ dml[x] for x in range(2)])
    rho = (cmat * ao[None]).sum(axis=2).astype(np.float64)
    grad = np.stack([[2 * (cmat[x] * dao[a]).sum(axis=1) for a in range(3)] for x in range(2)]).astype(np.float64)
    assert not rho[1].any() and not grad[1].any() and abs(dev.nelec_last - 1.0) < 1e-4
    vr, vec, exc, nelec, keep = xr.functional_reference(name, rho, grad, dev.weights, FLOOR)
    assert keep.sum() > npts // 2
    e_rel_host, e_rel_ref = abs(e_dev - e_host) / abs(e_host), xr.rel_err_scalar(e_dev, exc)
    v_ref, _ = xr.vmat_reference(ao.astype(np.float64), dao.astype(np.float64), vr.astype(np.float64), vec.astype(np.float64))
    v_ref = v_ref.astype(np.float64)
    dv_host = [np.abs(v_dev[x] - v_host[x]).max() / np.abs(v_host[x]).max() for x in range(2)]
    dv_ref = [np.abs(v_dev[x] - v_ref[x]).max() / np.abs(v_ref[x]).max() for x in range(2)]
    print(f"XCCHAIN {name} npts {npts} E_xc {e_dev:.12f} rel host {e_rel_host:.2e} ref {e_rel_ref:.2e} "
          f"v rel host {dv_host[0]:.2e} {dv_host[1]:.2e} ref {dv_ref[0]:.2e} {dv_ref[1]:.2e}")
    assert xr.rel_err_scalar(dev.nelec_last, nelec) < 1e-11
    assert e_rel_host < 1e-12 and e_rel_ref < 1e-11
    assert np.abs(v_ref[1]).max() > 1e-3  # the empty spin's potential is not small: it is what the defect hit
    assert max(dv_host) < 1e-10 and max(dv_ref) < 1e-10
