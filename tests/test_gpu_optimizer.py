"""The device-resident optimiser step on the MI355X: the re-pack against dqmc_set_weights at the default specs, fit_wf against
the host-path loop in float64, a float32 training run whose forward-Laplacian graph keeps being replayed, and a replayed
E_loc evaluation after a device update against a freshly created context."""

import numpy as np
import pytest
import torch

from deepqmc_amd import MolecularHamiltonian, Molecule
from deepqmc_amd.engine import Engine
from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.optimizer import AdamOptimizer
from deepqmc_amd.sampling import MoleculeIdxSampler, synthetic_walkers
from deepqmc_amd.spec import ANSATZES
from oracle import geom
from optimizer_util import (assert_same_answers, assert_same_buffers, check_fit_parity, host_path_loop, make_pair, moved_tree,
                            training_setup, update_both)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = [('paulinet', 'LiH'), ('ferminet', 'N2')]


@pytest.mark.parametrize('name,mol', CASES)
def test_device_repack_is_bit_identical_and_gives_the_same_answers_gpu(name, mol):
    """Checks 1 and 2 at the default specs in float32 with 4096 walkers.  LiH / PauliNet binds the generated sub-step kernel,
    so its tape is among the buffers; the local-energy call creates the float64 twins after the first device update, the second
    update rewrites them in place."""
    h, spec, tree, A, B = make_pair(name, mol, torch.float32, DEV)
    update_both(A, B, moved_tree(tree, 1, scale=0.02))
    need = (0, 1, 2) if A.substep_kernel() else (0, 2)
    assert_same_buffers(A, B, need=need)
    assert_same_answers(h, A, B, 4096)
    seen = assert_same_buffers(A, B, need=need + (3,))
    update_both(A, B, moved_tree(tree, 2, scale=0.02))
    assert assert_same_buffers(A, B, need=seen) == seen
    assert_same_answers(h, A, B, 4096, seed=9)


def test_fit_wf_matches_the_host_path_loop_gpu():
    """Check 5 in float64: 256 walkers, 10 steps, one state and two merged states.  Seed 3 and learning rate 5e-3 were chosen
    on the host path, through the emulated kernels at 48 walkers (mean loss of the first three steps -5.16, of the last three
    -6.59; 1e-2: -5.80 / -6.24; 2e-2 at 64 walkers: -5.60 / -5.71): the start is ~2 Ha above where Adam takes the energy within a
    few steps, far more than the sampling noise of 256 walkers."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = ANSATZES['paulinet']()
    check_fit_parity(h, spec, torch.float64, DEV, None, 1, 256, 10, 5e-3, 3)
    check_fit_parity(h, spec, torch.float64, DEV, None, 2, 256, 10, 5e-3, 3, merge_keys=['Jastrow'])


def _counters(wf, params):
    return [wf.engine(p).graph_counters() for p in params]


def test_training_run_replays_its_graph():
    """40 float32 steps of fit_wf with Adam at 4096 walkers: every E_loc mean is finite, and the forward-Laplacian graph of the
    context is captured at most twice per batch size and replayed ever after -- the property a host update destroys (each
    dqmc_set_weights drops the graphs; after eight captures the context runs eagerly for good).  The host-path loop runs
    beside it and its counters are printed, not asserted on."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = ANSATZES['paulinet']()
    wf, params, sampler, st = training_setup(h, spec, torch.float32, DEV, None, 1, 4096, 10, seed=3)
    means = []
    for _, state, _, stats in fit_wf(3, h, wf, AdamOptimizer(1e-3), MoleculeIdxSampler(0, 1, 1), sampler, range(40),
                                     TrainState(st, params, None), None):
        means.append(float(stats['local_energy/mean'].mean()))
    assert len(means) == 40 and np.isfinite(means).all(), means
    c = _counters(wf, params)[0]
    print('device path: E_loc mean', means[0], '->', means[-1], 'graph counters', c)
    assert c['captures'] <= 2 and c['replays'] > c['captures'], c
    wf_h, params_h, sampler_h, st_h = training_setup(h, spec, torch.float32, DEV, None, 1, 4096, 10, seed=3)
    losses = host_path_loop(3, h, wf_h, params_h, sampler_h, st_h, 40, 1e-3)
    print('host path:   E_loc mean', losses[0], '->', losses[-1], 'graph counters', _counters(wf_h, params_h)[0])


def test_replayed_graph_after_a_device_update_equals_a_fresh_context():
    """E_loc of 4096 walkers through the graph captured BEFORE a device update against a context created from the new values.
    "refine_probe" 0 freezes the refinement threshold, so that which walkers are re-evaluated in float64 is a function of the
    weights alone and not of how many calls a context has served."""
    h, spec, tree, A, _ = make_pair('paulinet', 'LiH', torch.float32, DEV)
    A.set_option('refine_probe', 0)
    r = torch.as_tensor(synthetic_walkers(h, 4096, seed=5), dtype=torch.float32, device=DEV)
    for _ in range(3):                       # eager, capture, replay
        A.local_energy(r, static_io=True)
    before = A.graph_counters()
    assert before['captures'] >= 1 and before['replays'] >= 1, before
    new = moved_tree(tree, 6, scale=0.02)
    A.set_params_flat(A.params_flat(new))
    e_replayed, _ = A.local_energy(r, static_io=True)
    after = A.graph_counters()
    assert after['captures'] == before['captures'] and after['replays'] == before['replays'] + 1, (before, after)
    fresh = Engine(spec, h, new, dtype=torch.float32, device=DEV, norm_eps=geom.F32_EPS)
    fresh.set_option('refine_probe', 0)
    e_fresh, _ = fresh.local_energy(r)
    assert torch.isfinite(e_replayed).all()
    assert torch.equal(e_replayed, e_fresh)
