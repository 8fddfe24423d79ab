"""Checks of the device-resident optimiser step (dqmc_set_param_map ... dqmc_apply_update, deepqmc_amd/optimizer.py, fit.py)
shared by the emulated CPU tests and the GPU tests."""
import copy
import dataclasses

import numpy as np
import torch

from deepqmc_amd.engine import Engine
from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.loss import compute_energy_loss_and_grad
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.optimizer import AdamOptimizer
from deepqmc_amd.params import init_params
from deepqmc_amd.pretrain import adam, apply_updates, merge_states
from deepqmc_amd.sampling import DecorrSampler, MoleculeIdxSampler, MultiElectronicStateSampler, MultiNuclearGeometrySampler, synthetic_walkers
from deepqmc_amd.spec import ANSATZES
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from oracle import geom

BUFFERS = {0: 'weights', 1: 'tape', 2: 'fused planes', 3: "twin's weights"}


def make_pair(name, molname, dtype, device, lib=None, seed=3, **spec_kw):
    """Two contexts A, B created from the same tree, and that tree."""
    h = MolecularHamiltonian(mol=Molecule.from_name(molname))
    spec = dataclasses.replace(ANSATZES[name](), **spec_kw)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    mk = lambda: Engine(spec, h, tree, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS)
    return h, spec, tree, mk(), mk()


def moved_tree(tree, seed, scale=0.05):
    rng = np.random.default_rng(seed)
    return {m: {k: np.asarray(v, np.float64) + scale * rng.normal(size=np.shape(v)) for k, v in leaves.items()} for m, leaves in tree.items()}


def update_both(A, B, tree):
    """A takes `tree` through the host path (compile + dqmc_set_weights), B through the device path."""
    A.set_params(tree)
    B.set_params_flat(B.params_flat(tree))


def assert_same_buffers(A, B, need=(0,)):
    """Every weight buffer both contexts have is byte-equal; those of `need` must exist.  Returns the buffers compared."""
    seen = []
    for which, label in BUFFERS.items():
        a, b = A.debug_read_weights(which), B.debug_read_weights(which)
        assert (a is None) == (b is None), label
        if a is None:
            assert which not in need, f'{label}: the context has no such buffer'
            continue
        assert a.size == b.size and a.size > 0, label
        assert np.array_equal(a, b), f'{label}: {int((a != b).sum())} of {a.size} bytes differ'
        seen.append(which)
    return seen


def assert_same_answers(h, A, B, n_walkers, seed=7, n_sub=2):
    """wf_eval, local_energy and one mcmc_steps call agree bit for bit: sign, log|psi|, E_loc, the accept bits, the moved walkers."""
    r = torch.as_tensor(synthetic_walkers(h, n_walkers, seed=seed), dtype=A.dtype, device=A.device)
    (sa, la), (sb, lb) = A.wf_eval(r), B.wf_eval(r)
    assert torch.equal(sa, sb) and torch.equal(la, lb)
    (ea, _), (eb, _) = A.local_energy(r), B.local_energy(r)
    assert torch.isfinite(ea).all() and torch.equal(ea, eb)
    out = []
    for eng, s, l in ((A, sa, la), (B, sb, lb)):
        st = {'r': r.clone(), 'log': l.clone(), 'sign': s.clone(), 'age': torch.zeros(n_walkers, dtype=torch.int32, device=eng.device),
              'tau': torch.full((1,), 0.3, dtype=eng.dtype, device=eng.device)}
        _, acc = eng.mcmc_steps(st, n_sub, seed=11, return_accept=True)
        out.append((st, acc))
    (sta, acca), (stb, accb) = out
    assert torch.equal(acca, accb)
    for k in ('r', 'log', 'sign', 'age', 'tau'):
        assert torch.equal(sta[k], stb[k]), k
    return ea


def training_setup(h, spec, dtype, device, lib, n_states, n_walkers, length, seed):
    wf = NeuralNetworkWaveFunction(h, spec, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS)
    params = [wf.init(seed + s, perturb_envelopes=0.1) for s in range(n_states)]
    sampler = MultiNuclearGeometrySampler(MultiElectronicStateSampler(DecorrSampler(h, wf, length=length, tau=0.3), n_states))
    R = torch.as_tensor(h.mol.coords, dtype=dtype, device=device)[None]
    smpl_state = sampler.init(seed, params, n_walkers, R)
    return wf, params, sampler, smpl_state


def host_path_loop(rng, h, wf, params, sampler, smpl_state, steps, lr, merge_keys=None):
    """The training loop written from the public host-path pieces: tree gradients, pretrain.adam on trees, apply_updates,
    wf.invalidate (recompile + dqmc_set_weights), sampler.update.  Returns the loss of every step."""
    opt = adam(lr)
    opt_state = [opt.init(p) for p in params]
    mis = MoleculeIdxSampler(0, 1, 1)
    losses = []
    for k in range(steps):
        seed = int(rng) * 1000003 + k
        smpl_state, pc, _ = sampler.sample(seed, smpl_state, params, mis.sample())
        loss, grads, _ = compute_energy_loss_and_grad(seed, h, wf, params, pc)
        for s, p in enumerate(params):
            upd, opt_state[s] = opt.update(grads[s], opt_state[s], p)
            apply_updates(p, upd)
        merge_states(params, merge_keys)
        for p in params:
            wf.invalidate(p)
        smpl_state = sampler.update(smpl_state, params)
        losses.append(float(loss))
    return losses


def device_path_loop(rng, h, wf, params, sampler, smpl_state, steps, lr, merge_keys=None, sync_every=None):
    losses = []
    state = TrainState(smpl_state, params, None)
    for _, state, _, stats in fit_wf(rng, h, wf, AdamOptimizer(lr), MoleculeIdxSampler(0, 1, 1), sampler, range(steps), state, merge_keys,
                                     sync_every=sync_every):
        losses.append(float(stats['local_energy/mean'].mean()))
    return losses, state


def flat(tree, prog):
    return prog.flatten_params(tree)


def check_fit_parity(h, spec, dtype, device, lib, n_states, n_walkers, steps, lr, seed, length=3, merge_keys=None, rtol=1e-10,
                     want_decrease=True):
    """fit_wf against the host-path loop from the same start: the loss of every step and the final parameters.  The host
    path's own trajectory must show the loss going down first (mean of the last steps below the mean of the first)."""
    wf_h, params_h, sampler_h, st_h = training_setup(h, spec, dtype, device, lib, n_states, n_walkers, length, seed)
    losses_h = host_path_loop(seed, h, wf_h, params_h, sampler_h, st_h, steps, lr, merge_keys)
    n_end = max(steps // 3, 1)
    print('host-path losses  ', losses_h)
    if want_decrease:
        assert np.mean(losses_h[-n_end:]) < np.mean(losses_h[:n_end]), losses_h
    wf_d, params_d, sampler_d, st_d = training_setup(h, spec, dtype, device, lib, n_states, n_walkers, length, seed)
    start = copy.deepcopy(params_d)
    losses_d, state = device_path_loop(seed, h, wf_d, params_d, sampler_d, st_d, steps, lr, merge_keys)
    print('device-path losses', losses_d)
    dev = max(abs(a - b) / abs(a) for a, b in zip(losses_h, losses_d))
    print('largest relative loss deviation', dev)
    assert dev <= rtol, (losses_h, losses_d)
    for s in range(n_states):
        assert state.params[s] is params_d[s]
        prog = wf_d.engine(params_d[s]).program
        th, td, t0 = flat(params_h[s], prog), flat(params_d[s], prog), flat(start[s], prog)
        assert np.abs(td - t0).max() > 0          # (the generator synced the leaves when it finished)
        err = np.abs(th - td).max() / np.abs(th).max()
        print(f'state {s}: final theta deviation {err:.2e} of max|theta|')
        assert err <= rtol, err
    return losses_h, losses_d
