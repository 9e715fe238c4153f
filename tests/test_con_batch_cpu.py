"""Batch proposals on a constrained model, the parts that need no GPU: (a) pybo_amd.propose_batch with
policy='cei' on a models.Constrained of ORACLE members -- the generic host path of pybo_amd/batch.py, every member observing each pick
at its own posterior mean -- against the from-scratch greedy of tests/con_batch_ref.py, with and without a feasible incumbent; (b) the
refusals that come before any index is built; (c) the CEI index still carries no `.batch`; (d) the chain of the device's scoring kernel
(pybo_amd/csrc/acq_core.h: con_chain) compiled with the host compiler, bit for bit against numpy's chain (tests/con_ref.py).

Tolerance of (a): the one the device is held to (con_batch_ref.val_tol: the members' stated tolerances propagated through the product).  Both
sides are the oracle's float64 arithmetic of the same formula on the same data and agree far better -- they differ only in that the
host path predicts a pick alone where the reference reads it out of the prediction of all of Z -- but the picks are compared exactly,
and a value cannot be right within that tolerance by accident."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import batch_ref
import con_batch_ref
import con_cases as cases
import con_ref
from oracle import gp_ref
from test_ens_prune_cpu import _special
import pybo_amd
from pybo_amd import models, policies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pybo_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'c', 'con_chain_check.cpp')
BOUNDS = np.array([[0.0, 1.0]] * 3)


@pytest.fixture(scope='module')
def small():
    """(problem, fitted models.Constrained over oracle members): N = 70, d = 3, J = 2, 500 candidates."""
    p = cases.build(70, 3, 'se', 3, 2, m=500)
    return p, _oracle_model(p)


def _oracle_model(p):
    obj = gp_ref.make_gp(*p['hypers'][0], p['kernel'])
    cons = [gp_ref.make_gp(*h, p['kernel']) for h in p['hypers'][1:]]
    model = models.Constrained(obj, cons, thresholds=p['thr'])
    model.add_data(p['X'], np.column_stack([p['y'], p['C']]))
    return model


def _check_host_path(p, model, policy, kind, target, nb, ref):
    hypers, _, params = con_batch_ref.members_of(p, kind)
    if kind is not None:
        params[0] = target
    before = [(m.X.copy(), m.Y.copy()) for m in model._members]
    Xq, vals, idx = pybo_amd.propose_batch(model, np.array([[0.0, 1.0]] * p['d']), p['X'], nb, policy=policy, xgrid=p['Z'])
    tol = con_batch_ref.val_tol(kind, params, hypers, ref['mu'], ref['s2'])
    print('margins', ref['margin'])
    print('idx', idx, ref['idx'])
    print('val err / tol', np.abs(vals - ref['val']) / tol)
    assert con_batch_ref.admitted(ref) and batch_ref.MIN_MARGIN == 1e-5      # the admission condition, on the reference itself
    np.testing.assert_array_equal(idx, ref['idx'])
    assert np.all(np.abs(vals - ref['val']) <= tol)
    np.testing.assert_array_equal(Xq, p['Z'][idx])
    # the caller's model is untouched: every member keeps its data
    assert model.ndata == len(p['X']) and all(np.array_equal(m.X, X0) and np.array_equal(m.Y, Y0) for m, (X0, Y0) in zip(model._members, before))
    # round 0 is the index's own best grid point
    v0 = model.get_constrained(target, p['Z'])
    assert idx[0] == gp_ref.topk_desc(v0, 1)[0] and vals[0] == v0[idx[0]]


def test_propose_batch_on_oracle_members_equals_the_from_scratch_greedy_with_an_incumbent(small):
    """'cei' with a feasible incumbent: the policy's own target (best posterior mean among the probably feasible observations)."""
    p, model = small
    target = policies.CEI(model, None, p['X']).acq[1]
    assert target is not None
    hypers, Y, params = con_batch_ref.members_of(p, 'ei')
    ref = con_batch_ref.greedy(p['X'], Y, p['Z'], p['kernel'], hypers, 'ei', [target] + params[1:], 6)
    _check_host_path(p, model, 'cei', 'ei', target, 6, ref)


def test_propose_batch_on_oracle_members_equals_the_from_scratch_greedy_without_an_incumbent():
    """'cei' while nothing qualifies as an incumbent (a pmin nobody reaches): the probability of feasibility alone, the shared case
    'se_j2_pof'.  The objective takes no part in the value; in the host path it still observes every pick (add_data takes 1 + J columns)."""
    p, kind, nb, ref = con_batch_ref.case('se_j2_pof')
    model = _oracle_model(p)
    assert kind is None and policies.CEI(model, None, p['X'], pmin=1.5).acq == ('cei', None)
    _check_host_path(p, model, ('cei', dict(pmin=1.5)), None, None, nb, ref)


def test_every_member_observes_a_pick_at_its_own_posterior_mean(small):
    """The believer step of the host path hands add_data ONE row of 1 + J values, the members' own means at the pick."""
    p, model = small
    seen = []

    class Spy(models.Constrained):
        def copy(self):
            c = Spy(self.objective.copy(), [m.copy() for m in self.constraints], self.thresholds.copy())
            return c

        def add_data(self, X, Y):
            seen.append((np.array(X), np.array(Y), [float(m.predict(X)[0][0]) for m in self._members]))
            models.Constrained.add_data(self, X, Y)

    spy = Spy(model.objective.copy(), [m.copy() for m in model.constraints], model.thresholds.copy())
    Xq, vals, idx = pybo_amd.propose_batch(spy, BOUNDS, p['X'], 3, policy='cei', xgrid=p['Z'])
    assert len(seen) == 2                                  # nb - 1 believer steps, none after the last pick
    for (x, y, means), i in zip(seen, idx):
        assert np.array_equal(x, p['Z'][i:i + 1]) and y.shape == (1, 3) and np.array_equal(y[0], means)
    assert len({round(float(v), 12) for v in seen[0][1][0]}) == 3      # three different members, three different means


def test_fantasies_and_pending_are_refused_before_an_index_is_built(small):
    p, model = small
    built = []

    def policy(model, bounds, X):
        built.append(1)
        return policies.CEI(model, bounds, X)

    with pytest.raises(ValueError, match='constrained'):
        pybo_amd.propose_batch(model, BOUNDS, p['X'], 4, policy=policy, xgrid=p['Z'], fantasies=8)
    with pytest.raises(ValueError, match='constrained'):
        pybo_amd.propose_batch(model, BOUNDS, p['X'], 4, policy=policy, xgrid=p['Z'], pending=[3])
    with pytest.raises(ValueError, match='constrained'):
        pybo_amd.propose_batch(model, BOUNDS, p['X'], 4, policy=policy, xgrid=p['Z'], fantasies=8, pending=[3])
    assert built == []
    pybo_amd.propose_batch(model, BOUNDS, p['X'], 2, policy=policy, xgrid=p['Z'])
    assert built == [1]


def test_the_cei_index_still_has_no_batch(small):
    p, model = small
    for kw in ({}, dict(pmin=1.5)):
        index = policies.CEI(model, None, p['X'], **kw)
        assert index.acq[0] == 'cei' and not hasattr(index, 'batch')
    # and an index of another kind on a constrained model is still refused by name
    with pytest.raises(ValueError, match='batch proposals need an EI, PI or UCB index'):
        from pybo_amd.batch import _score
        _score(model, 'ehvi', None, p['Z'])


# ---- (d) con_chain on the host --------------------------------------------------------------------------------------------------
def _compiler():
    for name in ('g++', 'c++', 'clang++'):
        path = shutil.which(name)
        if path:
            return path
    pytest.fail('no host C++ compiler (g++, c++ or clang++) to build tests/c/con_chain_check.cpp with')


def _build(directory, name, flags):
    exe = os.path.join(str(directory), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Wextra', '-Werror', '-ffp-contract=off'] + list(flags) + [SRC, '-o', exe])
    return exe


def _run(exe, *args):
    p = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == '', p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == 'con chain ok', lines[-3:]
    return [ln.split() for ln in lines[:-1]]


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('con_chain'), 'con_chain_check', ['-O2'])


def _chain_rows(exe, tmp_path, rows, has_obj):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    rows.tofile(src)
    out = _run(exe, src, dst, str(rows.shape[1]), str(int(has_obj)))
    assert out[-1] == ['rows', str(len(rows))]
    return np.fromfile(dst, dtype=np.float64)


def _same_bits(a, b):
    """bit for bit; any NaN equals any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64))


def test_the_chain_s_special_values_agree_with_numpy_bit_for_bit(exe):
    lines = [f for f in _run(exe) if f[0] == 'chain']
    assert len(lines) == 2 * 15 * 15
    for _, has_obj, t0, t1, r in lines:
        t0, t1, r = np.float64(float.fromhex(t0)), np.float64(float.fromhex(t1)), float.fromhex(r)
        want = con_ref.chain(t0, [t1]) if has_obj == '1' else con_ref.pof_chain([t0, t1])
        assert _same_bits([r], [want]), (has_obj, t0, t1, r, want)


@pytest.mark.parametrize('J', [1, 2, 3, 16])
def test_the_chain_agrees_with_numpy_bit_for_bit_from_both_starts(exe, tmp_path, J):
    """The value ranges of test_con_core_host.py: objective values over the whole range of non-negative doubles (0, denormals, +inf),
    probabilities uniform with the ends, factors above 1 (clamped) and NaN mixed in."""
    rng = np.random.RandomState(30 + J)
    m = 200000
    a = _special(rng, m)
    P = rng.rand(m, J)
    edge = rng.randint(0, 6, size=(m, J))
    P[edge == 0] = 1.0
    P[edge == 1] = 0.0
    P[edge == 2] = 1.0 + rng.rand(m, J)[edge == 2]
    nan = rng.rand(m) < 0.01
    P[nan, rng.randint(0, J, size=m)[nan]] = np.nan
    with_obj = _chain_rows(exe, tmp_path, np.column_stack([a, P]), 1)
    assert _same_bits(with_obj, con_ref.chain(a, list(P.T)))
    without = _chain_rows(exe, tmp_path, P, 0)
    assert _same_bits(without, con_ref.pof_chain(list(P.T)))
    assert np.all(np.isnan(with_obj[nan])) and np.all(np.isnan(without[nan]))
    fin = ~np.isnan(without)
    assert np.all(without[fin] <= 1.0) and np.all(without[fin] >= 0.0)      # a probability, whatever the factors were
    # a lone objective (no factor folded yet) keeps its bits
    assert _same_bits(_chain_rows(exe, tmp_path, a[:, None], 1), a)


def test_the_chain_check_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    san = _build(tmp_path, 'con_chain_check_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    _run(san)
    rows = np.column_stack([np.linspace(0.0, 2.0, 64), np.linspace(0.0, 1.5, 64), np.linspace(1.0, 0.0, 64)])
    assert len(_chain_rows(san, tmp_path, rows, 1)) == 64 and len(_chain_rows(san, tmp_path, rows, 0)) == 64


def test_the_kernel_calls_the_function_the_check_includes():
    import re
    assert '#include "../../pybo_amd/csrc/acq_core.h"' in open(SRC).read()
    bat = open(os.path.join(CSRC, 'kernels_batch.hip')).read()
    body = bat[bat.index('void k_con_batch_score'):bat.index('// The single-model pick')]
    assert body.count('con_chain(') == 1 and 'batch_score_frame(' in body and 'con_fold(' not in body and ' * ' not in body.replace('(int64_t)j * M', '')
    everything = '\n'.join(open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith(('.hip', '.h')))
    assert len(re.findall(r'^GPX_ACQ_FN[^\n(]*\bcon_chain\(', everything, flags=re.M)) == 1      # defined once
