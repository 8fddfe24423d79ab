"""The device-resident optimiser step through the SIMT emulation of the kernels: the re-pack of dqmc_weights_from_params
against dqmc_set_weights bit for bit, the transpose of the packing, Adam against pretrain._Adam, fit_wf against the host-path
loop, stale trees and the context cache, argument errors."""
import copy
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from deepqmc_amd.engine import DqmcError
from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.optimizer import AdamOptimizer, NaturalGradientOptimizer, NoOptimizer
from deepqmc_amd.pretrain import adam, apply_updates
from deepqmc_amd.sampling import MoleculeIdxSampler, synthetic_walkers
from deepqmc_amd.spec import ANSATZES
from optimizer_util import (assert_same_answers, assert_same_buffers, check_fit_parity, make_pair, moved_tree, training_setup,
                            update_both)
from simt_util import emu_lib

SMALL = dict(embedding_dim=32, n_interactions=1, n_determinants=2)
DTYPES = {'float32': torch.float32, 'float64': torch.float64}


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('name', ['paulinet', 'ferminet'])
def test_device_repack_is_bit_identical_and_gives_the_same_answers(name, dtype):
    """Checks 1 and 2 of the issue on a small ansatz: weights and fused planes after a device update equal those of the host
    path byte for byte -- with the float64 twin created AFTER the first update (it starts from the device's doubles) and
    updated in place by the second -- and wf_eval, local_energy and mcmc_steps agree bit for bit."""
    h, spec, tree, A, B = make_pair(name, 'LiH', DTYPES[dtype], 'cpu', emu_lib(), **SMALL)
    update_both(A, B, moved_tree(tree, 1))
    assert 2 in assert_same_buffers(A, B, need=(0, 2))
    assert_same_answers(h, A, B, 8)                  # (float32: the local-energy call creates the twins)
    seen = assert_same_buffers(A, B, need=(0, 2, 3) if dtype == 'float32' else (0, 2))
    update_both(A, B, moved_tree(tree, 2))
    assert assert_same_buffers(A, B, need=seen) == seen
    assert_same_answers(h, A, B, 8, seed=9)
    # the plan can be rebuilt after a device update (the host copy of the weights is stale by then): same planes again
    for eng in (A, B):
        eng.set_option('fused_wt', 2)
    assert_same_buffers(A, B, need=seen)
    # and the host path takes over again without a trace
    t3 = moved_tree(tree, 3)
    A.set_params(t3)
    B.set_params(t3)
    assert not B.params_ahead
    assert_same_buffers(A, B, need=seen)


def test_device_repack_of_the_default_lih_paulinet_covers_the_tape():
    """The default LiH / PauliNet spec in float32 binds the generated sub-step kernel: its weight tape (scaled tanh layers,
    bf16 planes, gathered tables) must come out of the device re-pack byte-equal too.  Creation and packing only."""
    h, spec, tree, A, B = make_pair('paulinet', 'LiH', torch.float32, 'cpu', emu_lib())
    assert A.lib.dqmc_substep_kernel(A._ctx, ctypes.create_string_buffer(128), 128) == 1
    update_both(A, B, moved_tree(tree, 4))
    assert assert_same_buffers(A, B, need=(0, 1, 2))[:3] == [0, 1, 2]


@pytest.mark.parametrize('name', ['paulinet', 'ferminet'])
def test_grad_to_params_is_unflatten_grad(name):
    h, spec, tree, A, _ = make_pair(name, 'LiH', torch.float64, 'cpu', emu_lib(), **SMALL)
    prog = A.program
    g = torch.as_tensor(np.random.default_rng(0).normal(size=prog.weights.size))
    got, again = A.grad_to_params(g), A.grad_to_params(g)
    assert torch.equal(got, again)
    ref = prog.flatten_params(prog.unflatten_grad(g))
    assert np.array_equal(got.numpy(), ref)
    # flatten_params is the inverse of unflatten_params, and params_flat reads the tree's values back from the weights
    assert np.array_equal(prog.flatten_params(prog.unflatten_params(ref)), ref)
    assert np.array_equal(A.params_flat().numpy(), prog.flatten_params(tree))


def test_adam_step_matches_pretrain_adam():
    """Ten steps on fixed random gradients against pretrain._Adam on trees.  Bound 1e-12 of max|theta|: unit roundoff x ~10
    operations x 10 steps plus FMA contraction, with ~100x margin.  Measured: 0 through the emulation (no FMA contraction on the host)."""
    h, spec, tree, A, B = make_pair('paulinet', 'LiH', torch.float64, 'cpu', emu_lib(), **SMALL)
    prog = A.program
    rng = np.random.default_rng(5)
    lr = lambda count: 1e-2 / (1 + count)
    host, opt = copy.deepcopy(tree), adam(lr, b1=0.8, b2=0.95, eps=1e-6)
    hstate = opt.init(host)
    theta = A.params_flat()
    mu, nu, norms = torch.zeros_like(theta), torch.zeros_like(theta), torch.zeros(3, dtype=torch.float64)
    for t in range(10):
        g = rng.normal(size=prog.n_params()) * 10.0 ** rng.integers(-6, 1, size=prog.n_params())
        gt = prog.unflatten_params(g)
        upd, hstate = opt.update(gt, hstate, host)
        ref_norms = [np.sqrt(sum(float(np.sum(np.square(x[m][k]))) for (m, k) in prog.grad_leaves)) for x in (host, gt, upd)]
        apply_updates(host, upd)
        A.adam_step(theta, mu, nu, torch.as_tensor(g), lr=lr(t), b1=0.8, b2=0.95, eps=1e-6, t=t + 1, norms=norms)
        np.testing.assert_allclose(norms.numpy(), ref_norms, rtol=1e-13, atol=0)
    ref = prog.flatten_params(host)
    err = np.abs(theta.numpy() - ref).max() / np.abs(ref).max()
    print('adam: largest deviation relative to max|theta|', err)
    assert err <= 1e-12
    np.testing.assert_allclose(mu.numpy(), prog.flatten_params(hstate['mu']), rtol=1e-12, atol=1e-300)
    # the step ends with the re-pack: the context now equals one that took the host's tree through set_params
    B.set_params({m: {k: prog.unflatten_params(theta)[m][k] if (m, k) in prog.grad_leaves else v for k, v in lv.items()}
                  for m, lv in tree.items()})
    assert_same_buffers(B, A, need=(0, 2))
    # apply_update: theta += scale * delta
    before, delta = theta.clone(), torch.as_tensor(rng.normal(size=prog.n_params()))
    A.apply_update(theta, delta, scale=-0.5, norms=norms)
    assert torch.equal(theta, before + (-0.5) * delta)
    np.testing.assert_allclose(norms.numpy(), [before.norm(), delta.norm(), 0.5 * delta.norm()], rtol=1e-13)


def _lih_small():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    return h, dataclasses.replace(ANSATZES['paulinet'](), **SMALL)


# seed and learning rate of the parity runs: chosen on the HOST path so that its loss goes down within the five steps
FIT_SEED, FIT_LR = 3, 2e-2


def test_fit_wf_matches_the_host_path_loop():
    h, spec = _lih_small()
    check_fit_parity(h, spec, torch.float64, 'cpu', emu_lib(), 1, 16, 5, FIT_LR, FIT_SEED)


def test_fit_wf_matches_the_host_path_loop_two_states_merged():
    h, spec = _lih_small()
    check_fit_parity(h, spec, torch.float64, 'cpu', emu_lib(), 2, 16, 5, FIT_LR, FIT_SEED, merge_keys=['Jastrow'])


def test_stale_trees_sync_and_cache_eviction():
    h, spec = _lih_small()
    wf, params, sampler, st = training_setup(h, spec, torch.float64, 'cpu', emu_lib(), 1, 8, 2, seed=1)
    tree = params[0]
    start = copy.deepcopy(tree)
    prog = wf.engine(tree).program
    same = lambda a, b: np.array_equal(prog.flatten_params(a), prog.flatten_params(b))
    gen = fit_wf(1, h, wf, AdamOptimizer(1e-2), MoleculeIdxSampler(0, 1, 1), sampler, range(3), TrainState(st, params, None), None)
    _, state, _, stats = next(gen)
    assert state.params[0] is tree and wf.params_stale(tree) and same(tree, start)      # stepped, leaves still old
    assert float(stats['opt/update_norm'][0]) > 0
    theta = state.opt[0]['theta'].numpy().copy()
    assert not np.array_equal(theta, prog.flatten_params(start))
    # another tree takes the only context; coming back must give the stepped values, not the stale leaves
    r = torch.as_tensor(synthetic_walkers(h, 4, seed=2))
    want = wf.engine(tree).wf_eval(r)[1].clone()
    wf.max_engines = 1
    eng0 = wf.engine(tree)
    other = wf.init(9, perturb_envelopes=0.1)
    assert wf.engine(other) is eng0 and not wf.params_stale(tree)
    assert np.array_equal(prog.flatten_params(tree), theta)                              # the eviction synced the tree
    assert torch.equal(wf.engine(tree).wf_eval(r)[1], want)
    gen.close()
    # sync_every=1 keeps the leaves current at every yield; the optimiser state carries the same values
    wf2, params2, sampler2, st2 = training_setup(h, spec, torch.float64, 'cpu', emu_lib(), 1, 8, 2, seed=1)
    for _, state, _, _ in fit_wf(1, h, wf2, AdamOptimizer(1e-2), MoleculeIdxSampler(0, 1, 1), sampler2, range(2),
                                 TrainState(st2, params2, None), None, sync_every=1):
        assert not wf2.params_stale(params2[0])
        assert np.array_equal(prog.flatten_params(params2[0]), state.opt[0]['theta'].numpy())
    # sync_params by hand, and a checkpoint never holds stale leaves
    wf3, params3, sampler3, st3 = training_setup(h, spec, torch.float64, 'cpu', emu_lib(), 1, 8, 2, seed=1)
    gen = fit_wf(1, h, wf3, AdamOptimizer(1e-2), MoleculeIdxSampler(0, 1, 1), sampler3, range(2), TrainState(st3, params3, None), None)
    _, state, _, _ = next(gen)
    assert wf3.params_stale(params3[0])
    wf3.sync_params(params3[0])
    assert not wf3.params_stale(params3[0]) and np.array_equal(prog.flatten_params(params3[0]), state.opt[0]['theta'].numpy())
    gen.close()


def test_checkpoint_save_syncs_stale_trees(tmp_path):
    from deepqmc_amd import checkpoint
    h, spec = _lih_small()
    wf, params, sampler, st = training_setup(h, spec, torch.float64, 'cpu', emu_lib(), 1, 8, 2, seed=1)
    gen = fit_wf(1, h, wf, AdamOptimizer(1e-2), MoleculeIdxSampler(0, 1, 1), sampler, range(2), TrainState(st, params, None), None)
    step, state, _, _ = next(gen)
    assert wf.params_stale(params[0])
    checkpoint.save(tmp_path / 'chk.pt', step, state, wf)
    assert not wf.params_stale(params[0])
    step2, loaded = checkpoint.load(str(tmp_path / 'chk.pt'))
    prog = wf.engine(params[0]).program
    assert step2 == step and np.array_equal(prog.flatten_params(loaded.params[0]), state.opt[0]['theta'].numpy())
    gen.close()


def test_other_optimizers_step():
    """NoOptimizer leaves the parameters alone; NaturalGradientOptimizer applies -lr x the flat natural gradient."""
    from deepqmc_amd.loss import compute_energy_loss_and_natgrad
    h, spec = _lih_small()
    wf, params, sampler, st = training_setup(h, spec, torch.float64, 'cpu', emu_lib(), 1, 8, 2, seed=1)
    start = copy.deepcopy(params[0])
    prog = wf.engine(params[0]).program
    for _, state, _, stats in fit_wf(1, h, wf, NoOptimizer(), MoleculeIdxSampler(0, 1, 1), sampler, range(1), TrainState(st, params, None), None):
        assert state.opt is None and not wf.params_stale(params[0]) and torch.isfinite(stats['local_energy/mean']).all()
    mis = MoleculeIdxSampler(0, 1, 1)
    _, pc, _ = sampler.sample(1 * 1000003, st, params, mis.sample())
    _, deltas, _ = compute_energy_loss_and_natgrad(1 * 1000003, h, wf, params, pc, damping=1e-2)
    ref = prog.flatten_params(start) - 0.05 * prog.flatten_params(deltas[0])
    opt = NaturalGradientOptimizer(0.05, damping=1e-2)
    for _, state, _, stats in fit_wf(1, h, wf, opt, MoleculeIdxSampler(0, 1, 1), sampler, range(1), TrainState(st, params, None), None):
        np.testing.assert_allclose(state.opt[0]['theta'].numpy(), ref, rtol=1e-9, atol=1e-12)
    assert np.array_equal(prog.flatten_params(params[0]), state.opt[0]['theta'].numpy())


def test_argument_errors():
    h, spec, tree, A, _ = make_pair('paulinet', 'LiH', torch.float64, 'cpu', emu_lib(), **SMALL)
    lib, prog = A.lib, A.program
    theta = A.params_flat(tree)

    def expect_arg_error(rc):
        assert rc == -1 and len(lib.dqmc_last_error()) > 0      # DQMC_E_ARG and a message

    expect_arg_error(lib.dqmc_weights_from_params(A._ctx, theta.data_ptr()))                       # before a map is set
    expect_arg_error(lib.dqmc_grad_to_params(A._ctx, theta.data_ptr(), theta.data_ptr()))
    src = np.ascontiguousarray(prog.grad_src, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    expect_arg_error(lib.dqmc_set_param_map(A._ctx, p(src[:-4]), src.size - 4, prog.n_params()))   # wrong length
    bad = src.copy()
    bad[np.nonzero(src >= 0)[0][0]] = prog.n_params()
    expect_arg_error(lib.dqmc_set_param_map(A._ctx, p(bad), bad.size, prog.n_params()))            # index out of range
    expect_arg_error(lib.dqmc_weights_from_params(A._ctx, theta.data_ptr()))                       # (neither call set a map)
    out = np.empty(prog.weights.size * 8 - 8, np.uint8)
    expect_arg_error(lib.dqmc_debug_read_weights(A._ctx, 0, out.ctypes.data_as(ctypes.c_void_p), out.size))   # size mismatch
    assert lib.dqmc_debug_read_weights(A._ctx, 3, None, 0) == -4 and A.debug_read_weights(3) is None           # no twin: UNSUPPORTED
    with pytest.raises(DqmcError):
        A.set_params_flat(theta[:-1].contiguous())
    A.set_params_flat(theta)                                                                       # the lazy map upload
    assert lib.dqmc_weights_from_params(A._ctx, theta.data_ptr()) == 0
