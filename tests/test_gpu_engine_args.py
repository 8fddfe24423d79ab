"""The Engine facade's argument checks on the MI355X: host tensors and a wrong walker shape are refused before the library is
reached (a guard stands in for it, so a broken check fails the test instead of handing a host pointer to a kernel), and the
engine then repeats its earlier results bit for bit."""
import pytest
import torch

from deepqmc_amd.engine import DqmcError
from engine_args_util import guarded
from pretrain_util import make

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = 8


def test_host_tensors_and_bad_walkers_never_reach_the_device():
    h, spec, tree, eng, r = make('paulinet', 'LiH', B, DEV, dtype=torch.float32)
    eng.set_option('refine_probe', 0)          # (fixed refinement threshold: a repeated call flags the same walkers)
    r = torch.as_tensor(r, dtype=torch.float32, device=DEV)
    sign0, log0 = eng.wf_eval(r)
    e0, _ = eng.local_energy(r)
    cpu_state = {'r': r.cpu(), 'log': log0.clone(), 'sign': sign0.clone(), 'age': torch.zeros(B, dtype=torch.int32, device=DEV),
                 'tau': torch.full((1,), 0.3, dtype=torch.float32, device=DEV)}
    with guarded(eng):
        for call in (lambda: eng.set_params_flat(torch.zeros(eng.program.n_params(), dtype=torch.float64)),
                     lambda: eng.energy_record(e0.cpu()),
                     lambda: eng.mcmc_steps(cpu_state, 1),
                     lambda: eng.psi_and_grad(torch.zeros(B, eng.N + 1, 3, dtype=torch.float32, device=DEV))):
            with pytest.raises(DqmcError):
                call()
    sign1, log1 = eng.wf_eval(r)
    e1, _ = eng.local_energy(r)
    assert torch.equal(sign1, sign0) and torch.equal(log1, log0) and torch.equal(e1, e0)
