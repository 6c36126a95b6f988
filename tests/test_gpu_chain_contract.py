"""The chain-resident kernels against the host restatement of their arithmetic contract
(tests/chain_contract.py), BIT FOR BIT:

    linear_chain_kernel    binf_hmc_sample_linear_f64, binf_gibbs_linear_sample_n_f64
    poly_chain_kernel      binf_hmc_sample_poly_f64, binf_gibbs_poly_sample_n_f64
    hmc_poly_small_kernel  binf_hmc_sample_poly_f64 under MODE_LANE_PER_CHAIN

Every state, accept flag, counter, recorded precision and adapted step equals the
restatement's in every chain.  The energies equal the restatement evaluated with ONE value of
``log tau`` per chain and sweep: the correctly rounded logarithm or one of its two neighbours
(the device library's log is within an ulp; at tau = 1 only 0.0).  All draws are supplied, so
no stream is involved; tests/test_chain_contract.py has shown on the host that no accept test
of these cases is within 8 ulp of a tie and that the restatement itself is exact on integer
data and inside the derived force bound otherwise.

The shapes are the smallest at which each mechanism runs (chain_contract.N_LIST and the K
lists): every KMAX instantiation, both round interleaves, the three force variants of the
polynomial kernel, sequential / one-leaf / regular / ragged trees, 1, 5 and 300 chains."""
import numpy as np
import pytest
import torch

import chain_contract as CC
from binf_amd import _native

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Equal bit for bit; two NaNs count as equal whatever their payload."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def dev(a, device, dtype=torch.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device).to(dtype)


def prior_args(c, device):
    if c['prior'] is None:
        return None, None, True
    mu, var, first = c['prior']
    return dev(mu, device), dev(var, device), first


def hmc_run(device, c, layout=None, design=None):
    """One launch of the single-transition entry point of a layout: (q, acc, e_before, e_after)."""
    layout = layout or c['layout']
    C, K = c['theta'].shape
    q0, q_out = dev(c['theta'], device), torch.zeros((C, K), dtype=torch.float64, device=device)
    acc = torch.zeros(C, dtype=torch.uint8, device=device)
    eb, ea = torch.zeros(C, dtype=torch.float64, device=device), torch.zeros(C, dtype=torch.float64, device=device)
    tau = c['tau'] if np.isscalar(c['tau']) else dev(c['tau'], device)
    dtc = None if np.isscalar(c['dt']) else dev(c['dt'], device)
    mu, var, first = prior_args(c, device)
    mode = _native.MODE_FMA if c['fused'] else _native.MODE_EXACT
    design = c['design'] if design is None else design
    if layout == 'linear':
        fn = _native.hmc_sample_linear
    else:
        fn = _native.hmc_sample_poly
        mode |= _native.MODE_LANE_PER_CHAIN if layout == 'lane' else 0
    fn(q0, dev(c['p0'], device), dev(c['u'], device), q_out, acc, None, eb, ea, dev(design, device),
       dev(c['ys'], device), tau, mu, var, first, dev(c['pre'], device), dev(c['post'], device),
       float(c['dt']) if dtc is None else 0.0, dtc, c['L'], False, 1.05, 0.95, mode)
    torch.cuda.synchronize()
    return q_out.cpu().numpy(), acc.cpu().numpy().astype(bool), eb.cpu().numpy(), ea.cpu().numpy()


def check_energies(eb, ea, t, what):
    """Each chain's two energies are the restatement's under one and the same candidate of
    ``log tau``; returns how many chains needed a neighbour of the correctly rounded one."""
    ok = same(t['e_before'], eb) & same(t['e_after'], ea)                  # [3 x C]
    bad = np.nonzero(~ok.any(axis=0))[0]
    assert len(bad) == 0, (what, bad[:5], eb[bad[:5]], t['e_before'][:, bad[:5]], ea[bad[:5]], t['e_after'][:, bad[:5]])
    return int((~ok[0]).sum())


def check_transition(got, c, t, what):
    q, acc, eb, ea = got
    assert np.array_equal(acc, t['acc'][0]), (what, np.nonzero(acc != t['acc'][0])[0][:5])
    want = np.where(t['acc'][0][:, None], t['prop'], c['theta'])
    diff = np.nonzero(~same(q, want).all(axis=1))[0]
    assert len(diff) == 0, (what, 'chains', diff[:5], q[diff[:2]], want[diff[:2]])
    return check_energies(eb, ea, t, what)


# ---------------------------------------------------------------------------
# 1. one transition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('layout,i', CC.hmc_case_ids())
def test_one_transition_is_the_restatement_bit_for_bit(device, layout, i):
    c = CC.hmc_case(layout, i)
    if CC.tree_height(c['N']) > CC.MAX_HEIGHT:
        # N = 1023: numpy's tree for it is four levels deep (1023 -> 504 + 519 -> ... -> 64 + 71), more
        # than a chain's 64 lanes hold; the entry points must decline it, not run another order
        assert not _native.linear_resident_supported(c['K'], c['N'])
        with pytest.raises(NotImplementedError):
            hmc_run(device, c)
        return
    t = CC.hmc_expect(c)
    assert np.all(t['tie_free']) and np.all(t['acc'] == t['acc'][0])
    what = '%s K=%d N=%d C=%d L=%d %s' % (layout, c['K'], c['N'], c['C'], c['L'], 'fma' if c['fused'] else 'exact')
    nb = check_transition(hmc_run(device, c), c, t, what)
    if np.isscalar(c['tau']) and c['tau'] == 1.0:
        assert np.all(CC.log_candidates(np.ones(1)) == 0.0) and nb == 0
    print('%s: %d of %d chains took a neighbour of the correctly rounded log tau; %d accepted'
          % (what, nb, c['C'], int(t['acc'][0].sum())))


# ---------------------------------------------------------------------------
# 2. Gibbs sweeps
# ---------------------------------------------------------------------------
def gibbs_run(device, c):
    C, K, n = c['C'], c['K'], c['n']
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=device)
    o = dict(theta=z(C, K), tau=z(C), rc=z(n, C, K), rt=z(n, C), eb=z(n, C), ea=z(n, C),
             acc=torch.zeros((n, C), dtype=torch.uint8, device=device),
             nacc=torch.zeros(C, dtype=torch.int64, device=device))
    mu, var, first = prior_args(c, device)
    hmc = c['move'] == 'hmc'
    o['dt'] = dev(c['dt'], device) if hmc else None
    fn = _native.gibbs_linear_sample_n if c['layout'] == 'linear' else _native.gibbs_poly_sample_n
    fn(dev(c['theta'], device), dev(c['tau'], device), o['theta'], o['tau'], dev(c['design'], device),
       dev(c['ys'], device), n, 1, move=_native.MOVE_HMC if hmc else _native.MOVE_RWMC,
       mode=_native.MODE_FMA if c['fused'] else _native.MODE_EXACT, nsteps=c['L'], timestep=0.0, dt_chain=o['dt'],
       n_adapt=c['n_adapt'], uprate=CC.UPRATE, downrate=CC.DOWNRATE, stepsize=c.get('stepsize', 0.0),
       prior_means=mu, prior_vars=var, prior_first=first, gp_where=c['gp_where'], gp_shape=CC.GP_SHAPE,
       gp_rate=CC.GP_RATE, gamma_shape=c['gamma_shape'], gamma_rate=CC.GAMMA_RATE, rec_coefficients=o['rc'],
       rec_precision=o['rt'], accepted=o['acc'], n_accepted=o['nacc'], e_before=o['eb'] if hmc else None,
       e_after=o['ea'] if hmc else None, p0=dev(c['p0'], device), u=dev(c['u'], device), g=dev(c['g'], device),
       keep_precision=c['keep_tau'])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items() if v is not None}


@pytest.mark.parametrize('layout,move,i', CC.gibbs_case_ids())
def test_gibbs_sweeps_are_the_restatement_bit_for_bit(device, layout, move, i):
    c = CC.gibbs_case(layout, move, i)
    t = CC.gibbs_expect(c)
    assert t['tie_free'] and t['flags_agree']
    o = gibbs_run(device, c)
    what = '%s %s K=%d N=%d C=%d n=%d' % (layout, move, c['K'], c['N'], c['C'], c['n'])
    assert np.array_equal(o['acc'].astype(bool), t['acc']), what
    assert np.array_equal(o['nacc'], t['n_accepted']), what
    assert same(o['rc'], t['theta']).all(), (what, np.nonzero(~same(o['rc'], t['theta']).all(axis=2)))
    assert same(o['rt'], t['tau']).all(), (what, np.nonzero(~same(o['rt'], t['tau'])))
    assert same(o['theta'], t['theta'][-1]).all() and same(o['tau'], t['tau'][-1]).all(), what
    if c['keep_tau']:
        assert same(o['rt'], np.broadcast_to(c['tau'], o['rt'].shape)).all()
    nb = 0
    if move == 'hmc':
        assert same(o['dt'], t['dt']).all(), what
        assert not np.any(o['dt'] == c['dt'])                 # two sweeps of adaption moved every step
        for s in range(c['n']):
            nb += check_energies(o['eb'][s], o['ea'][s], dict(e_before=t['e_before'][s], e_after=t['e_after'][s]),
                                 '%s sweep %d' % (what, s))
    print('%s: %d of %d chain-sweeps took a neighbour of the correctly rounded log tau; %d accepted'
          % (what, nb, c['n'] * c['C'], int(t['acc'].sum())))


# ---------------------------------------------------------------------------
# 3. cross-checks between the kernels
# ---------------------------------------------------------------------------
def expect(c):
    """The restated transition; its accept tests are clear of ties whatever candidate of log tau
    (tests/test_chain_contract.py shows the same on the host for every case used here)."""
    t = CC.hmc_expect(c)
    assert np.all(t['tie_free']) and np.all(t['acc'] == t['acc'][0])
    return t


@pytest.mark.parametrize('K,N', CC.CROSS_SHAPES)
def test_stored_powers_and_running_products_are_two_contracts_each_met(device, K, N):
    """The linear kernel given the polynomial design matrix uses stored powers where the
    polynomial kernel uses running products: each equals ITS restatement."""
    c, lin = CC.cross_cases(K, N)
    check_transition(hmc_run(device, c), c, expect(c), 'poly')
    check_transition(hmc_run(device, lin), lin, expect(lin), 'linear on the polynomial design')


@pytest.mark.parametrize('N', CC.ONE_COEFFICIENT_N)
def test_with_one_coefficient_the_three_kernels_agree(device, N):
    """K = 1: the mock datum is theta_0 under either contract, so chi^2 -- and with it E_before
    -- agrees bit for bit between the three kernels.  The two group layouts share the force
    order as well: their whole transition agrees.  One lane per chain sums the force
    sequentially, so its trajectory (and E_after) is its own; it is held to its restatement."""
    cases = CC.one_coefficient_cases(N)
    assert np.array_equal(cases[1]['design'], np.ones((1, N))) and cases[0]['C'] in CC.CHAINS
    got = [hmc_run(device, c) for c in cases]
    for c, g in zip(cases, got):
        check_transition(g, c, expect(c), '%s K=1 N=%d' % (c['layout'], N))
    for a, b in zip(got[0], got[1]):
        assert same(a, b).all()
    for g in got[2:]:
        assert same(g[2], got[0][2]).all()


# ---------------------------------------------------------------------------
# 4. a non-finite coefficient
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [np.nan, np.inf])
@pytest.mark.parametrize('layout,K,N', CC.NON_FINITE_SHAPES)
def test_a_non_finite_coefficient_poisons_its_own_chain_only(device, layout, K, N, bad):
    c_bad = 2
    c = CC.non_finite_case(layout, K, N)
    C, theta = c['C'], c['theta']
    clean = expect(c)
    c['theta'] = theta.copy()
    c['theta'][c_bad, K - 1] = bad
    q, acc, eb, ea = hmc_run(device, c)
    # its energies are NaN (an infinite coefficient: E_before is +inf, NaN from the first force on)
    assert np.isnan(ea[c_bad]) and (np.isnan(eb[c_bad]) if np.isnan(bad) else eb[c_bad] == np.inf)
    assert not acc[c_bad] and same(q[c_bad], c['theta'][c_bad]).all()
    keep = np.arange(C) != c_bad
    t = {k: (v[..., keep] if k in ('e_before', 'e_after', 'acc') else v[keep]) for k, v in clean.items()
         if k in ('e_before', 'e_after', 'acc', 'prop')}
    check_transition((q[keep], acc[keep], eb[keep], ea[keep]), dict(theta=theta[keep]), t, layout)
