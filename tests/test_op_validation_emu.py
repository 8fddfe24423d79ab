"""Engine::validate (deepqmc_amd/csrc/engine_program.inl) pinned op kind by op kind: one slot of one op of a valid program is
corrupted at a time (slot numbers of include/dqmc.h) and dqmc_create must answer `malformed op #<index> kind <kind>`
before it plans or launches anything.  CPU only: the emulated library runs the same host code."""
import copy
import dataclasses

import pytest
import torch

from deepqmc_amd.engine import DqmcError, Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.program import N_OP_I, compile_program
from deepqmc_amd.spec import paulinet
from simt_util import emu_lib
from test_psiformer_emu import small_psiformer

FEAT_EN, FEAT_EE, LINEAR, SPIN_MEAN, CONV, ROW_SUM, ORBITALS, SLOGDET, FINAL, ATTENTION = 1, 2, 3, 4, 5, 7, 8, 9, 10, 11
BAD_BUF = 10_000
KINDS = {'paulinet': {FEAT_EN, FEAT_EE, LINEAR, SPIN_MEAN, CONV, ROW_SUM, ORBITALS, SLOGDET, FINAL},
         'psiformer': {FEAT_EN, LINEAR, ORBITALS, SLOGDET, FINAL, ATTENTION}}

# (op kind, what is wrong, slot, value(program, op.i))
CASES = [
    (FEAT_EN, 'dst buf out of range', 0, lambda p, i: BAD_BUF),
    (FEAT_EN, 'dst buf negative', 0, lambda p, i: -1),
    (FEAT_EE, 'dst buf out of range', 0, lambda p, i: BAD_BUF),
    (FEAT_EE, 'table offset negative', 1, lambda p, i: -1),
    (FEAT_EE, 'pair table past the end', 1, lambda p, i: p.itable.size),
    (FEAT_EE, 'row count differs from the buffer', 2, lambda p, i: i[2] + 1),
    (LINEAR, 'no pieces', 0, lambda p, i: 0),
    (LINEAR, 'five pieces', 0, lambda p, i: 5),
    (LINEAR, 'src buf out of range', 1, lambda p, i: BAD_BUF),
    (LINEAR, 'src buf negative', 1, lambda p, i: -1),
    (LINEAR, 'K = 0', 3, lambda p, i: 0),
    (LINEAR, 'K wider than the src buf', 3, lambda p, i: p.bufs[i[1]][1] + 1),
    (LINEAR, 'src r0 negative', 2, lambda p, i: -1),
    (LINEAR, 'src rows overflow', 2, lambda p, i: p.bufs[i[1]][0] - i[20] + 1),
    (LINEAR, 'dst buf out of range', 17, lambda p, i: BAD_BUF),
    (LINEAR, 'dst r0 negative', 18, lambda p, i: -1),
    (LINEAR, 'dst rows overflow', 18, lambda p, i: p.bufs[i[17]][0] - i[20] + 1),
    (LINEAR, 'dst col0 not a multiple of 4', 19, lambda p, i: i[19] + 2),
    (LINEAR, 'dst columns overflow', 19, lambda p, i: p.bufs[i[17]][1]),
    (LINEAR, 'nout wider than the dst buf', 21, lambda p, i: p.bufs[i[17]][1] + 1),
    (LINEAR, 'weight offset negative', 22, lambda p, i: -4),
    (LINEAR, 'weight offset not a multiple of 4', 22, lambda p, i: i[22] + 1),
    (LINEAR, 'weight offset past the end', 22, lambda p, i: p.weights.size // 4 * 4),
    (LINEAR, 'bias offset past the end', 23, lambda p, i: p.weights.size // 4 * 4),
    (LINEAR, 'activation 5', 24, lambda p, i: 5),
    (LINEAR, 'activation negative', 24, lambda p, i: -1),
    (LINEAR, 'residual buf out of range', 25, lambda p, i: BAD_BUF),
    (SPIN_MEAN, 'src buf out of range', 0, lambda p, i: BAD_BUF),
    (SPIN_MEAN, 'dst buf out of range', 1, lambda p, i: BAD_BUF),
    (SPIN_MEAN, 'dst buf without two rows', 1, lambda p, i: i[0]),
    (CONV, 'edge buf out of range', 0, lambda p, i: BAD_BUF),
    (CONV, 'node buf out of range', 1, lambda p, i: BAD_BUF),
    (CONV, 'dst buf out of range', 2, lambda p, i: BAD_BUF),
    (CONV, 'dst columns overflow', 3, lambda p, i: p.bufs[i[2]][1]),
    (CONV, 'table past the end', 4, lambda p, i: p.itable.size),
    (CONV, 'width wider than the edge buf', 6, lambda p, i: p.bufs[i[0]][1] + 4),
    (ROW_SUM, 'src buf out of range', 0, lambda p, i: BAD_BUF),
    (ROW_SUM, 'dst buf with more than one row', 1, lambda p, i: i[0]),
    (ORBITALS, 'backflow buf out of range', 0, lambda p, i: BAD_BUF),
    (ORBITALS, 'dst buf out of range', 1, lambda p, i: BAD_BUF),
    (ORBITALS, 'envelope weights past the end', 2, lambda p, i: p.weights.size),
    (ORBITALS, 'envelope weight offset negative', 5, lambda p, i: -1),
    (ORBITALS, 'n_env negative', 6, lambda p, i: -1),
    (SLOGDET, 'orbital buf out of range', 0, lambda p, i: BAD_BUF),
    (SLOGDET, 'orbital buf too narrow', 0, lambda p, i: 0),
    (FINAL, 'jastrow buf out of range', 0, lambda p, i: BAD_BUF),
    (FINAL, 'conf_coeff past the end', 1, lambda p, i: p.weights.size),
    (FINAL, 'cusp kind 3', 2, lambda p, i: 3),
    (FINAL, 'alphas past the end', 3, lambda p, i: p.weights.size - 1),
    (FINAL, 'alphas offset negative', 3, lambda p, i: -1),
    (ATTENTION, 'q buf out of range', 0, lambda p, i: BAD_BUF),
    (ATTENTION, 'dst buf out of range', 3, lambda p, i: BAD_BUF),
    (ATTENTION, 'no heads', 4, lambda p, i: 0),
    (ATTENTION, 'head_dim 0', 5, lambda p, i: 0),
    (ATTENTION, 'heads wider than the buffers', 4, lambda p, i: p.bufs[i[0]][1] // i[5] + 1),
    (ATTENTION, 'n_const negative', 6, lambda p, i: -1),
    (ATTENTION, 'constant keys past the end', 6, lambda p, i: p.weights.size),
]

_cache = {}


def setup(name):
    if name not in _cache:
        spec = paulinet() if name == 'paulinet' else small_psiformer()
        h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
        tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=5, perturb_envelopes=0.1)
        _cache[name] = spec, h, tree, compile_program(spec, tree, h.n_up, h.n_down, h.n_nuc)
    return _cache[name]


def create(name, program):
    spec, h, tree, _ = setup(name)
    return Engine(spec, h, tree, dtype=torch.float64, device='cpu', lib=emu_lib(), compiler=lambda params: program)


@pytest.mark.parametrize('name', sorted(KINDS))
def test_valid_program_builds(name):
    program = setup(name)[3]
    assert {op.kind for op in program.ops} == KINDS[name]
    create(name, program).close()


@pytest.mark.parametrize('name,kind,what,slot,value',
                         [pytest.param(n, *c, id=f'{n}-kind{c[0]}-{c[1].replace(" ", "_")}') for n in sorted(KINDS) for c in CASES
                          if c[0] in KINDS[n]])
def test_corrupted_slot_is_rejected(name, kind, what, slot, value):
    base = setup(name)[3]
    k = next(j for j, op in enumerate(base.ops) if op.kind == kind)
    ops = copy.deepcopy(base.ops)
    ops[k].i = list(ops[k].i) + [0] * (N_OP_I - len(ops[k].i))
    ops[k].i[slot] = int(value(base, ops[k].i))
    assert ops[k].i[slot] != (list(base.ops[k].i) + [0] * N_OP_I)[slot], what
    with pytest.raises(DqmcError, match=rf'malformed op #{k} kind {kind}$'):
        create(name, dataclasses.replace(base, ops=ops))
