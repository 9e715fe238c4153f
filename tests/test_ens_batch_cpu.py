"""Batch proposals on the ensemble, the parts that need no GPU: the reference of tests/ens_batch_ref.py against batch_ref with one
member, the admission of every case, the hook MCMC only offers over device members, and the new entry of the ABI."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_ref
import ens_batch_ref
from oracle import gp_ref
from helpers import synth_problem

import pybo_amd
from pybo_amd import _lib, batch, models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('tag', ['se_300_3_ei', 'matern1_130_5_pi', 'matern5_256_2_ucb'])
def test_one_member_is_the_single_model_greedy(tag):
    prob, ref = batch_ref.case(tag)
    hypers = ens_batch_ref.member_hypers(prob['ell'], 1)
    (ell, rho, sn2, bias), = hypers
    np.testing.assert_array_equal(ell, prob['ell'])
    assert (rho, sn2, bias) == (prob['rho'], prob['sn2'], prob['bias'])
    param = ens_batch_ref.ensemble_param(prob['X'], prob['y'], prob['kernel'], hypers, prob['kind'])
    assert param == prob['param']
    got = ens_batch_ref.greedy(prob['X'], prob['y'], prob['Z'], prob['kernel'], hypers, prob['kind'], param, prob['nb'])
    np.testing.assert_array_equal(got['idx'], ref['idx'])
    np.testing.assert_array_equal(got['s2'][0], ref['s2'])
    np.testing.assert_array_equal(got['mu'][0], ref['mu_pick'])
    if prob['kind'] == 'ucb':
        # the mixture form of ONE member passes through (s2 + mu^2) - mu^2: a few roundings of mu^2 (<= 1.5^2) against s2 >= 1e-4
        np.testing.assert_allclose(got['val'], ref['val'], rtol=1e-11)
        np.testing.assert_allclose(got['margin'], ref['margin'], rtol=1e-4)
    else:
        np.testing.assert_array_equal(got['val'], ref['val'])
        np.testing.assert_array_equal(got['margin'], ref['margin'])


@pytest.mark.parametrize('tag', sorted(ens_batch_ref.CASES))
def test_every_case_is_admitted(tag):
    prob, ref = ens_batch_ref.case(tag)
    print(tag, 'min margin %.2g' % ref['margin'].min())
    assert ref['margin'].min() >= batch_ref.MIN_MARGIN
    assert len(set(ref['idx'].tolist())) == prob['nb']
    assert ref['mu'].shape == ref['s2'].shape == (len(prob['hypers']), prob['nb'])


def test_an_ensemble_over_host_members_keeps_the_generic_path(monkeypatch):
    X, y, ell = synth_problem(30, 2, seed=3)
    gp = gp_ref.make_gp(1e-3, 1.0, ell, 0.0)
    gp.add_data(X, y)
    mc = models.MCMC(gp, n=2, burn=2, rng=0)
    assert not hasattr(mc, 'acq_batch')
    with pytest.raises(AttributeError):
        mc.acq_batch
    calls = []
    host = batch._host_batch
    monkeypatch.setattr(batch, '_host_batch', lambda *a: calls.append(a[1]) or host(*a))
    Z = np.random.RandomState(1).rand(50, 2)
    Xq, vals, idx = pybo_amd.propose_batch(mc, [[0.0, 1.0]] * 2, X, 2, policy='ei', xgrid=Z, rng=0)
    assert calls == ['ei'] and len(set(idx.tolist())) == 2 and Xq.shape == (2, 2)


def test_the_entry_point_is_bound_and_exported_by_both_libraries():
    assert 'gpx_ensemble_sweep_batch' in _lib.SYMBOLS
    for name in ('libgpx.so', 'libgpx_diag.so'):
        lib = C.CDLL(os.path.join(ROOT, 'pybo_amd', 'csrc', name))
        assert hasattr(lib, 'gpx_ensemble_sweep_batch'), name
    assert callable(_lib.Engine.ensemble_batch)
