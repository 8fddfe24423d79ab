"""Compile (AnsatzSpec, parameter tree) into the flat layer program of include/dqmc.h.

The reference builds its forward pass by tracing haiku modules
(wf/nn_wave_function.py:127-173 -> wf/omni.py:157-178 -> gnn/electron_gnn.py:403-432);
here the same dataflow is emitted once, on the host, as a list of `dqmc_op` records over
per-walker activation buffers plus one contiguous weight buffer and one int table
(edge orderings of gnn/graph.py:17-31,132-139).  The HIP library executes the list.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .params import attention_feature_name, GNN, OMNI, WF, layer_dims, layer_name
from .spec import AnsatzSpec, MLPSpec

OP_FEAT_EN, OP_FEAT_EE, OP_LINEAR, OP_SPIN_MEAN, OP_CONV, OP_EDGE_SUM, OP_ROW_SUM = 1, 2, 3, 4, 5, 6, 7
OP_ORBITALS, OP_SLOGDET, OP_FINAL, OP_ATTENTION, OP_CONST = 8, 9, 10, 11, 12
ACT = {None: 0, 'tanh': 1, 'silu': 2, 'ssp': 3, 'mult_tanh': 4}
N_OP_I = 28


def pad4(n: int) -> int:
    return (n + 3) // 4 * 4


class DqmcBuf(ctypes.Structure):
    _fields_ = [('rows', ctypes.c_int32), ('width', ctypes.c_int32)]


class DqmcOp(ctypes.Structure):
    _fields_ = [('kind', ctypes.c_int32), ('i', ctypes.c_int32 * N_OP_I), ('f', ctypes.c_float * 4)]


class DqmcSystem(ctypes.Structure):
    _fields_ = [('n_up', ctypes.c_int32), ('n_down', ctypes.c_int32), ('n_nuc', ctypes.c_int32),
                ('n_det', ctypes.c_int32), ('dtype', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('norm_eps', ctypes.c_double), ('e_nuc', ctypes.c_double)]


@dataclass
class Op:
    kind: int
    i: List[int]
    f: List[float] = field(default_factory=lambda: [0.0] * 4)
    note: str = ''


def edge_pairs(n_up: int, n_down: int, edge_types: Sequence[str], self_interaction: bool):
    """(recv, send) of every edge row, in `single_array` order, per edge type
    (gnn/graph.py:17-31,132-139,246-335).  Returns {type: [(recv, send), ...]}."""
    N = n_up + n_down

    def block(senders, receivers, mask_self):
        ns, nr = len(senders), len(receivers)
        out = []
        if mask_self:
            assert ns == nr
            for k in range(ns - 1):                 # row k of the [n-1, n] edge array
                for rr in range(nr):
                    out.append((receivers[rr], senders[k + (1 if rr <= k else 0)]))
        else:
            for s in range(ns):
                for rr in range(nr):
                    out.append((receivers[rr], senders[s]))
        return out

    up, dn, al = list(range(n_up)), list(range(n_up, N)), list(range(N))
    res = {}
    for t in edge_types:
        if t == 'same':
            res[t] = block(up, up, not self_interaction) + block(dn, dn, not self_interaction)
        elif t == 'anti':
            res[t] = block(dn, up, False) + block(up, dn, False)     # du then ud
        elif t == 'up':
            res[t] = block(up, al, False)
        elif t == 'down':
            res[t] = block(dn, al, False)
        else:
            raise ValueError(t)
    return res


@dataclass
class Program:
    spec: AnsatzSpec
    n_up: int
    n_down: int
    n_nuc: int
    bufs: List[Tuple[int, int]]
    ops: List[Op]
    weights: np.ndarray            # float64
    itable: np.ndarray             # int32
    buf_names: Dict[str, int]
    weight_slots: List[tuple]      # (offset, module, leaf, kind, meta) for repacking
    flops_per_walker: float        # F_lin = 2 * sum rows*in*out over Linear layers (unpadded)
    # inverse of the weight packing: grad_src[j] = the parameter element flat weight j was copied from (-1: constant or
    # padding), element ids index the leaves of grad_leaves {(module, leaf): (first id, shape)}; grad_unsupported names a
    # packing that is not a copy (then the flat gradient cannot be mapped back)
    grad_src: Optional[np.ndarray] = None
    grad_leaves: Optional[Dict[Tuple[str, str], Tuple[int, tuple]]] = None
    grad_unsupported: Optional[str] = None
    # compile_program(..., nuclear_reverse=True): the nuclear-token stream as the library folds it on the device
    # (dqmc_set_nuclear_stream): {'n_layers', 'heads', 'dim', 'n_det', 'n_env', 'n_edge_lin', 'n_embed_lin', 'n_mlp_lin',
    # 'lin': [(w, b, n_in, n_out, act)] offsets into theta, 'zbias': (up, down), 'nuc_types', 'R', 'n_derived',
    # 'sc_row', 'sc_col': CSR of the weight entries that are copies of each derived element}.  Its leaves (nuclei_embedding,
    # nuclear_gnn_head) are part of grad_leaves without a copy in the weight buffer; the transpose of the fold exists on the
    # device only (Engine.grad_to_params).
    nuclear_stream: Optional[dict] = None
    # library option "nuclear_params" of the context this program was compiled for (Engine.set_option keeps it current): the
    # stream's parameter partials exist per walker, on the device
    nuclear_params: bool = False

    PER_WALKER_NUCLEAR = ('the nuclear-token stream has no per-walker partials (all walkers share it: one nuclear backward per '
                          'walker); only the walker-summed gradients (log_psi_vjp, orbitals_vjp, pretraining, AdamOptimizer) run '
                          'with nuclear tokens, and with nuclear_coords=True the coordinate calls (log_psi_grad_coords, '
                          'make_grad_nuc_log_wf, the AC-ZB / AC-ZVQZB forces); nuclear_params=True forms the stream\'s parameter '
                          'partials per walker on the device and opens log_psi_jacobian, log_psi_kfac, NaturalGradientOptimizer and '
                          'KFACOptimizer')

    def unflatten_grad(self, g):
        """Flat gradient over the weight buffer (dqmc_log_psi_vjp) -> haiku tree {module: {leaf: array}}: the transpose of
        the packing (copies, zero padding, broadcasts and column scatters are summed back onto their parameter element)."""
        if self.grad_unsupported:
            raise NotImplementedError(f'unflatten_grad: unsupported for this program ({self.grad_unsupported})')
        if self.nuclear_stream is not None:
            raise NotImplementedError('unflatten_grad: the transpose of the nuclear-stream fold runs on the device only; use '
                                      'Engine.grad_to_params(g) and Program.unflatten_params')
        if hasattr(g, 'detach'):
            g = g.detach().cpu().numpy()
        g = np.asarray(g, np.float64).reshape(-1)
        if g.size != self.grad_src.size:
            raise ValueError(f'gradient of {g.size} entries for a weight buffer of {self.grad_src.size}')
        n_el = sum(int(np.prod(sh)) for _, sh in self.grad_leaves.values())
        m = self.grad_src >= 0
        flat = np.zeros(n_el)
        np.add.at(flat, self.grad_src[m], g[m])
        tree: Dict[str, Dict[str, np.ndarray]] = {}
        for (mod, leaf), (base, shape) in self.grad_leaves.items():
            tree.setdefault(mod, {})[leaf] = flat[base:base + int(np.prod(shape))].reshape(shape)
        return tree

    def leaf_slices(self):
        """Columns of unflatten_jacobian per parameter leaf: {(module, leaf): (slice, shape)}, in grad_leaves order."""
        return {key: (slice(base, base + int(np.prod(shape))), tuple(shape)) for key, (base, shape) in self.grad_leaves.items()}

    def n_params(self):
        return sum(int(np.prod(sh)) for _, sh in self.grad_leaves.values())

    def unflatten_params(self, v):
        """A [n_params] vector (one row of unflatten_jacobian, or anything in its column order) -> haiku tree
        {module: {leaf: ndarray}}."""
        if hasattr(v, 'detach'):
            v = v.detach().cpu().numpy()
        v = np.asarray(v).reshape(-1)
        if v.size != self.n_params():
            raise ValueError(f'vector of {v.size} entries for {self.n_params()} parameters')
        tree: Dict[str, Dict[str, np.ndarray]] = {}
        for (mod, leaf), (sl, shape) in self.leaf_slices().items():
            tree.setdefault(mod, {})[leaf] = v[sl].reshape(shape)
        return tree

    def flatten_params(self, tree):
        """The inverse of unflatten_params: a haiku tree {module: {leaf: array}} -> float64 [n_params] vector in grad_leaves
        order (the theta of dqmc_weights_from_params).  Leaves the program does not read are ignored."""
        if self.grad_unsupported:
            raise NotImplementedError(f'flatten_params: unsupported for this program ({self.grad_unsupported})')
        out = np.empty(self.n_params(), np.float64)
        for (mod, leaf), (sl, shape) in self.leaf_slices().items():
            v = np.asarray(tree[mod][leaf], np.float64)
            if tuple(v.shape) != tuple(shape):
                raise ValueError(f'leaf {mod}:{leaf} has shape {tuple(v.shape)}, the program was compiled for {tuple(shape)}')
            out[sl] = v.reshape(-1)
        return out

    def _jacobian_gather(self):
        """Per source multiplicity m, the flat weight entries that hold the m-th copy of each parameter element (ascending
        entry order, as np.add.at in unflatten_grad sums them) and the mask of elements that have one."""
        if getattr(self, '_jac_gather', None) is None:
            n_el = self.n_params()
            j = np.nonzero(self.grad_src >= 0)[0]           # ascending
            e = self.grad_src[j]
            order = np.argsort(e, kind='stable')            # by element, ascending entry within an element
            j, e = j[order], e[order]
            first = np.searchsorted(e, np.arange(n_el))
            rank = np.arange(e.size) - first[e]
            tabs = []
            for m in range(int(rank.max()) + 1 if rank.size else 0):
                sel = rank == m
                idx = np.zeros(n_el, np.int64)
                has = np.zeros(n_el, bool)
                idx[e[sel]] = j[sel]
                has[e[sel]] = True
                tabs.append((idx, has))
            self._jac_gather = tabs
        return self._jac_gather

    def unflatten_jacobian(self, J):
        """Per-walker Jacobian over the weight buffer (Engine.log_psi_jacobian, [B, n_weights]) -> [B, n_params] on J's device
        and in J's dtype: row b is unflatten_grad(J[b]) flattened in grad_leaves order (see leaf_slices / unflatten_params).
        A gather per source multiplicity summed in a fixed order, so the result is deterministic on the GPU."""
        if self.grad_unsupported:
            raise NotImplementedError(f'unflatten_jacobian: unsupported for this program ({self.grad_unsupported})')
        if self.nuclear_stream is not None:
            raise NotImplementedError(f'unflatten_jacobian: {self.PER_WALKER_NUCLEAR}; the per-walker transpose of the '
                                      'nuclear-stream fold runs on the device only: use Engine.jacobian_to_params(J, logpsi, sign)')
        import torch
        if J.dim() != 2 or J.shape[1] != self.grad_src.size:
            raise ValueError(f'Jacobian of shape {tuple(J.shape)} for a weight buffer of {self.grad_src.size}')
        out = None
        for idx, has in self._jacobian_gather():
            col = J.index_select(1, torch.as_tensor(idx, device=J.device))
            if not has.all():
                col = torch.where(torch.as_tensor(has, device=J.device)[None], col, torch.zeros((), dtype=J.dtype, device=J.device))
            out = col if out is None else out.add_(col)
        if out is None:
            out = torch.zeros(J.shape[0], self.n_params(), dtype=J.dtype, device=J.device)
        return out

    def kfac_layout(self):
        """The layout of dqmc_log_psi_kfac's outputs (include/dqmc.h), computed from the program: {'n_linear', 'n_factor_doubles',
        'n_rest', 'rest_index': the flat weight entries of the rest columns (ascending), 'ops': one dict per LINEAR op in program
        order with 'op' (index into ops), 'module', 'nrows', 'has_bias', 'd_a', 'd_g' and the offsets 'a_off', 'g_off' of A_l
        and G_l in the factor buffer}."""
        owned = np.zeros(self.weights.size, bool)
        slot_mod = {sl[0]: sl[1] for sl in self.weight_slots}
        ops, off = [], 0
        for k, op in enumerate(self.ops):
            if op.kind != OP_LINEAR:
                continue
            i = op.i
            rows = sum(pad4(i[3 + 4 * p]) for p in range(i[0]))
            has_bias = i[23] >= 0
            d_a, d_g = rows + int(has_bias), pad4(i[21])
            owned[i[22]:i[22] + rows * d_g] = True
            if has_bias:
                owned[i[23]:i[23] + d_g] = True
            ops.append(dict(op=k, module=slot_mod.get(i[22], op.note), nrows=i[20], has_bias=has_bias, d_a=d_a, d_g=d_g, a_off=off, g_off=off + d_a * d_a))
            off += d_a * d_a + d_g * d_g
        rest = np.nonzero(~owned)[0]
        return dict(n_linear=len(ops), n_factor_doubles=off, n_rest=int(rest.size), rest_index=rest, ops=ops)

    def kfac_blocks(self):
        """The LINEAR ops grouped by haiku module, for Kronecker-factored preconditioning.  Returns (blocks, fallback):
        blocks = {module: {'ops': [indices into kfac_layout()['ops']], 'rows': [per op: int array over the op's d_A rows of A,
        the module's w row (bias: n_in) or -1 for padding], 'cols': [per op: int array over its ldw columns of G, the w column
        or -1], 'n_in', 'n_out', 'has_bias', 'R': total rows per walker of the module's ops}}, built from grad_src; every op's
        maps are checked to be permutations of the module's w rows (+ bias) and columns.  fallback = the names of the modules
        with a 'w' leaf that is not mapped this way (no op, or an op that covers only part of w): their parameters take the
        diagonal treatment."""
        if self.grad_unsupported:
            raise NotImplementedError(f'kfac_blocks: unsupported for this program ({self.grad_unsupported})')
        if self.nuclear_stream is not None and not self.nuclear_params:
            raise NotImplementedError(f'kfac_blocks: {self.PER_WALKER_NUCLEAR}')
        lay = self.kfac_layout()
        by_mod: Dict[str, list] = {}
        for q, o in enumerate(lay['ops']):
            by_mod.setdefault(o['module'], []).append(q)
        blocks, fallback = {}, []
        for (mod, leaf), (base, shape) in self.grad_leaves.items():
            if leaf != 'w':
                continue
            if mod not in by_mod or len(shape) != 2:
                fallback.append(mod)
                continue
            n_in, n_out = shape
            b_base = self.grad_leaves[(mod, 'b')][0] if (mod, 'b') in self.grad_leaves else None
            ok, rows_l, cols_l = True, [], []
            for q in by_mod[mod]:
                o = lay['ops'][q]
                i = self.ops[o['op']].i
                ldw, wr = o['d_g'], o['d_a'] - int(o['has_bias'])
                if o['has_bias'] != (b_base is not None):
                    ok = False
                    break
                src = self.grad_src[i[22]:i[22] + wr * ldw].reshape(wr, ldw)
                rel = np.where(src >= 0, src - base, -1)
                if ((src >= 0) & ((rel < 0) | (rel >= n_in * n_out))).any():
                    ok = False
                    break
                rows = np.full(o['d_a'], -1, np.int64)
                cols = np.full(ldw, -1, np.int64)
                rr, cc = np.nonzero(src >= 0)
                k_in, k_out = rel[rr, cc] // n_out, rel[rr, cc] % n_out
                # every packed row holds one w row, every packed column one w column, consistently
                rows[:wr][rr] = k_in
                cols[cc] = k_out
                if not (np.array_equal(rows[rr], k_in) and np.array_equal(cols[cc], k_out)):
                    ok = False
                    break
                if o['has_bias']:
                    bsrc = self.grad_src[i[23]:i[23] + ldw]
                    if not np.array_equal(bsrc >= 0, cols >= 0) or not np.array_equal(bsrc[cols >= 0] - b_base, cols[cols >= 0]):
                        ok = False
                        break
                    rows[wr] = n_in
                full_r = np.sort(rows[:wr][rows[:wr] >= 0])
                full_c = np.sort(cols[cols >= 0])
                if not (np.array_equal(full_r, np.arange(n_in)) and np.array_equal(full_c, np.arange(n_out))
                        and rr.size == n_in * n_out):
                    ok = False
                    break
                rows_l.append(rows)
                cols_l.append(cols)
            if not ok:
                fallback.append(mod)
                continue
            blocks[mod] = dict(ops=by_mod[mod], rows=rows_l, cols=cols_l, n_in=n_in, n_out=n_out, has_bias=b_base is not None,
                               R=sum(lay['ops'][q]['nrows'] for q in by_mod[mod]))
        return blocks, fallback

    def c_bufs(self):
        arr = (DqmcBuf * len(self.bufs))()
        for k, (r, w) in enumerate(self.bufs):
            arr[k].rows, arr[k].width = r, w
        return arr

    def c_ops(self):
        arr = (DqmcOp * len(self.ops))()
        for k, op in enumerate(self.ops):
            arr[k].kind = op.kind
            ii = list(op.i) + [0] * (N_OP_I - len(op.i))
            for j in range(N_OP_I):
                arr[k].i[j] = int(ii[j])
            for j in range(4):
                arr[k].f[j] = float(op.f[j])
        return arr


class _Builder:
    def __init__(self, spec, params, n_up, n_down, n_nuc):
        self.spec, self.params = spec, params
        self.n_up, self.n_down, self.n_nuc = n_up, n_down, n_nuc
        self.N = n_up + n_down
        self.bufs: List[Tuple[int, int]] = []
        self.names: Dict[str, int] = {}
        self.ops: List[Op] = []
        self.w: List[np.ndarray] = []
        self.w_len = 0
        self.slots: List[tuple] = []
        self.it: List[int] = []
        self.flops = 0.0
        # inverse of the packing (Program.grad_src / grad_leaves)
        self.src: List[np.ndarray] = []
        self.leaves: Dict[Tuple[str, str], Tuple[int, tuple]] = {}
        self.n_el = 0
        self.id_override: Dict[Tuple[str, str], np.ndarray] = {}
        self.grad_unsupported: Optional[str] = None
        self.dsrc: List[np.ndarray] = []      # per push_w: the derived element of the nuclear stream every entry is a copy of (-1: none)
        self.nuclear_stream: Optional[dict] = None

    def ids(self, module, leaf):
        """Element ids of parameter leaf (module, leaf), shaped like the leaf (or as overridden by a re-layout)."""
        key = (module, leaf)
        if key in self.id_override:
            return self.id_override[key]
        if key not in self.leaves:
            shape = tuple(np.shape(self.params[module][leaf]))
            self.leaves[key] = (self.n_el, shape)
            self.n_el += int(np.prod(shape))
        base, shape = self.leaves[key]
        return base + np.arange(int(np.prod(shape))).reshape(shape)

    def finish(self, prog: 'Program') -> 'Program':
        prog.grad_src = np.concatenate(self.src).astype(np.int64)
        prog.grad_leaves = dict(self.leaves)
        prog.grad_unsupported = self.grad_unsupported
        if self.nuclear_stream is not None:
            ns = dict(self.nuclear_stream)
            dsrc = np.concatenate(self.dsrc)
            j = np.nonzero(dsrc >= 0)[0]
            order = np.argsort(dsrc[j], kind='stable')        # by derived element, ascending entry within an element
            counts = np.bincount(dsrc[j], minlength=ns['n_derived'])
            assert counts.size == ns['n_derived'] and counts.min() >= 1
            ns['sc_row'] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            ns['sc_col'] = j[order].astype(np.int32)
            prog.nuclear_stream = ns
        return prog

    # -- allocation helpers --
    def buf(self, name, rows, width):
        self.bufs.append((max(rows, 1), pad4(width)))     # an empty edge segment (e.g. one electron per spin) keeps a dummy row
        self.names[name] = len(self.bufs) - 1
        return len(self.bufs) - 1

    def push_w(self, arr, slot, src=None, derived=None):
        """src: parameter element id of every entry of `arr` (-1: none); default: the leaf itself for 'raw' slots, none
        for constants.  derived: the element of the nuclear stream's derived vector every entry is a copy of."""
        off = self.w_len
        a = np.asarray(arr, np.float64).reshape(-1)
        n = pad4(a.size)
        buf = np.zeros(n)
        buf[:a.size] = a
        if src is None and slot[2] == 'raw':
            src = self.ids(slot[0], slot[1])
        sb = np.full(n, -1, np.int64)
        if src is not None:
            sb[:a.size] = np.asarray(src, np.int64).reshape(-1)
        self.src.append(sb)
        db = np.full(n, -1, np.int64)
        if derived is not None:
            db[:a.size] = np.asarray(derived, np.int64).reshape(-1)
        self.dsrc.append(db)
        self.w.append(buf)
        self.w_len += n
        self.slots.append((off,) + slot)
        return off

    def push_table(self, ints):
        off = len(self.it)
        self.it += [int(x) for x in ints]
        return off

    def pack_linear(self, module, piece_K: Sequence[int]):
        """W [sum pad4(K_p)][pad4(Nout)] with the rows of each concat piece padded."""
        p = self.params[module]
        W = np.asarray(p['w'], np.float64)
        assert W.shape[0] == sum(piece_K), (module, W.shape, piece_K)
        nout = W.shape[1]
        W_id = self.ids(module, 'w')
        blocks, sblocks, o = [], [], 0
        for K in piece_K:
            blk = np.zeros((pad4(K), pad4(nout)))
            blk[:K, :nout] = W[o:o + K]
            sblk = np.full((pad4(K), pad4(nout)), -1, np.int64)
            sblk[:K, :nout] = W_id[o:o + K]
            blocks.append(blk)
            sblocks.append(sblk)
            o += K
        w_off = self.push_w(np.concatenate(blocks, 0), (module, 'w', 'linear_w', tuple(piece_K)), np.concatenate(sblocks, 0))
        b_off = -1
        if 'b' in p:
            b = np.zeros(pad4(nout))
            b[:nout] = np.asarray(p['b'], np.float64)
            sb = np.full(pad4(nout), -1, np.int64)
            sb[:nout] = self.ids(module, 'b')
            b_off = self.push_w(b, (module, 'b', 'linear_b', (nout,)), sb)
        return w_off, b_off, nout

    def linear(self, module, pieces, dst, dst_r0, dst_col0, nrows, act, res=-1, res_r0=0, res_scale=1.0, note=''):
        """pieces: [(src buf, r0, K, bcast)]."""
        assert 1 <= len(pieces) <= 4
        w_off, b_off, nout = self.pack_linear(module, [p[2] for p in pieces])
        i = [len(pieces)]
        for p in pieces:
            i += list(p)
        i += [0] * (17 - len(i))
        i += [dst, dst_r0, dst_col0, nrows, nout, w_off, b_off, ACT[act], res, res_r0, int(res_scale != 1.0)]
        if nrows == 0:          # empty segment: the weights stay in the buffer (parameter order), no op
            return nout
        self.ops.append(Op(OP_LINEAR, i, [0, 0, 0, 0], note or module))
        self.flops += 2.0 * nrows * sum(p[2] for p in pieces) * nout
        return nout

    def mlp(self, prefix, mspec: MLPSpec, pieces, in_dim, out_dim, dst, dst_r0, dst_col0, nrows, tmp_rows,
            res=-1, res_r0=0, res_scale=1.0):
        """hkext.MLP as a chain of LINEAR ops; hidden activations go to fresh buffers with
        `tmp_rows` rows per walker (row offsets preserved).  The residual applies to the
        last layer only (it wraps the whole MLP, hkext.py:130-137)."""
        for step in self.mlp_steps(prefix, mspec, pieces, in_dim, out_dim, dst, dst_r0, dst_col0, nrows, tmp_rows,
                                   res, res_r0, res_scale):
            step()

    def mlp_steps(self, prefix, mspec: MLPSpec, pieces, in_dim, out_dim, dst, dst_r0, dst_col0, nrows, tmp_rows,
                  res=-1, res_r0=0, res_scale=1.0):
        """The LINEAR ops of one MLP as a list of thunks, so that independent MLPs can be emitted
        in lockstep (ops of equal depth adjacent => one dependency level in the fused kernel).
        Hidden buffers hold just the `nrows` rows of the segment (`tmp_rows` is unused)."""
        dims = mspec.dims(in_dim, out_dim)
        state = {'cur': pieces}
        steps = []
        for k, dim in enumerate(dims):
            last = k == len(dims) - 1
            act = mspec.layer_act(k, len(dims))

            def step(k=k, dim=dim, last=last, act=act):
                if last:
                    self.linear(f'{prefix}/linear_{k}', state['cur'], dst, dst_r0, dst_col0, nrows, act, res, res_r0, res_scale)
                else:
                    hb = self.buf(f'{prefix}/hidden_{k}', nrows, dim)
                    self.linear(f'{prefix}/linear_{k}', state['cur'], hb, 0, 0, nrows, act)
                    state['cur'] = [(hb, 0, dim, 0)]
            steps.append(step)
        return steps

    @staticmethod
    def lockstep(*chains):
        for k in range(max(len(c) for c in chains)):
            for c in chains:
                if k < len(c):
                    c[k]()


def _nuclear_stream_descriptor(b: '_Builder', spec: AnsatzSpec, R, n_nuc: int) -> dict:
    """The stream of nuclear_stream.fold as offsets into theta (registers the nuclei_embedding / nuclear_gnn_head leaves and the
    shared attention leaves in grad_leaves)."""
    from .nuclear_stream import NUC_EDGE_MLP, NUC_EMB, NUC_HEAD, nuc_embed_mlp
    D, K = spec.embedding_dim, spec.n_determinants
    lin = []

    def add(module, act):
        w = b.ids(module, 'w')
        has_b = 'b' in b.params[module]
        lin.append((int(w.reshape(-1)[0]), int(b.ids(module, 'b').reshape(-1)[0]) if has_b else -1, int(w.shape[0]), int(w.shape[1]),
                    ACT[act]))

    def add_mlp(prefix, mspec, in_dim, out_dim):
        dims = mspec.dims(in_dim, out_dim)
        for i in range(len(dims)):
            add(f'{prefix}/linear_{i}', mspec.layer_act(i, len(dims)))
        return len(dims)

    n_edge = add_mlp(f'{NUC_EMB}/edge_mlp', NUC_EDGE_MLP, 4 + n_nuc, 32)
    n_embed = add_mlp(f'{NUC_EMB}/embed_mlp', nuc_embed_mlp(D), 32, D)
    n_mlp = 0
    for l in range(spec.n_interactions):
        uf = f'{layer_name(l)}/~/{attention_feature_name(spec)}'
        for nm in ('query', 'key', 'value', 'linear'):
            add(f'{uf}/multi_head_attention/{nm}', None)
        n_mlp = add_mlp(f'{uf}/mlp', spec.attn_mlp, D, D)
    n_env, zbias = 0, (-1, -1)
    if spec.envelope == 'simplified':
        n_env = spec.n_envelope_per_nucleus
        for glu in ('zetas_readout_glu', 'zetas_readout_glu_1'):
            for nm in ('W', 'V'):
                add(f'{NUC_HEAD}/{glu}/{nm}', None)
        zbias = tuple(int(b.ids(NUC_HEAD, f'zetas_bias_{spin}').reshape(-1)[0]) for spin in ('up', 'down'))
    n_derived = 2 * spec.n_interactions * n_nuc * D + (2 * n_nuc * K * n_env if n_env else 0)
    return dict(n_layers=spec.n_interactions, heads=spec.num_heads, dim=D, n_det=K, n_env=n_env, n_edge_lin=n_edge,
                n_embed_lin=n_embed, n_mlp_lin=n_mlp, lin=lin, zbias=zbias, nuc_types=np.asarray(spec.nuc_types, np.int32),
                R=np.ascontiguousarray(R, np.float64).reshape(n_nuc, 3), n_derived=n_derived)


def compile_program(spec: AnsatzSpec, params, n_up: int, n_down: int, n_nuc: int, R=None, eps=None, nuclear_reverse=False) -> Program:
    """`R` [n_nuc,3] and the safe-norm `eps` are needed only by ansatzes with nuclear tokens, whose
    electron-independent nuclear stream is folded into constants here (nuclear_stream.py).  `nuclear_reverse`: the program also
    describes that stream for the library (Program.nuclear_stream), which then folds it on the device after a device update
    and transposes it in Engine.grad_to_params; grad_unsupported stays unset and grad_leaves covers the stream's leaves."""
    b = _Builder(spec, params, n_up, n_down, n_nuc)
    nuc_kv, nuc_zetas = None, None
    if spec.nuclei_tokens:
        if R is None or eps is None:
            raise ValueError(f'{spec.name}: the nuclear geometry R and eps are needed to compile nuclear tokens')
        from .nuclear_stream import fold
        nuc_kv, nuc_zetas = fold(params, spec, R, eps)
        if nuclear_reverse:
            b.nuclear_stream = _nuclear_stream_descriptor(b, spec, R, n_nuc)
        else:
            b.grad_unsupported = 'the nuclear-token stream is folded into constants and simplified envelopes (not a copy of parameters)'
    N, K, D, E = n_up + n_down, spec.n_determinants, spec.embedding_dim, spec.two_particle_dim
    S2 = 1.0 / np.sqrt(2.0)

    # ---- input features ----
    d0, rows = layer_dims(spec, n_nuc)
    x = b.buf('x_feat', N, d0)
    b.ops.append(Op(OP_FEAT_EN, [x, int(spec.emb_log_rescale), int(spec.emb_use_spin)], note='electron-nucleus features'))
    x_dim = d0
    if spec.emb_project:
        x1 = b.buf('x0', N, D)
        b.linear(f'{GNN}/~/electron_embedding/linear', [(x, 0, d0, 0)], x1, 0, 0, N, None)
        x, x_dim = x1, D
    else:
        b.names['x0'] = x

    pairs = edge_pairs(n_up, n_down, spec.edge_types, spec.self_interaction)
    seg, n_edge_rows = {}, 0                      # edge type -> (row offset, n rows)
    for t in spec.edge_types:
        seg[t] = (n_edge_rows, len(pairs[t]))
        n_edge_rows += len(pairs[t])
    e, e_dim = -1, 0
    conv_tab: Dict[str, Tuple[int, int]] = {}
    if spec.edge_types:
        flat = [v for t in spec.edge_types for pr in pairs[t] for v in pr]
        tab = b.push_table(flat)
        e = b.buf('e0', n_edge_rows, 4)
        e_dim = 4
        b.ops.append(Op(OP_FEAT_EE, [e, tab, n_edge_rows, int(spec.edge_log_rescale)], note='electron-electron edge features'))
        for t in spec.edge_types:                 # per-receiver (edge row, sender) lists
            per = [[] for _ in range(N)]
            for k, (rc, sd) in enumerate(pairs[t]):
                per[rc].append((seg[t][0] + k, sd))
            S = max(len(p) for p in per)
            flat = []
            for p in per:
                p = p + [(-1, -1)] * (S - len(p))
                flat += [v for pr in p for v in pr]
            conv_tab[t] = (b.push_table(flat), S)

    # ---- interaction layers ----
    for l, row in enumerate(rows):
        ln = layer_name(l)
        if spec.layer_kind == 'attention':
            uf = f'{ln}/~/{attention_feature_name(spec)}'
            H = spec.num_heads
            hd = x_dim // H
            q, k_, v = (b.buf(f'l{l}/{nm}', N, H * hd) for nm in ('q', 'k', 'v'))
            for nm, dst in (('query', q), ('key', k_), ('value', v)):
                b.linear(f'{uf}/multi_head_attention/{nm}', [(x, 0, x_dim, 0)], dst, 0, 0, N, None)
            att = b.buf(f'l{l}/att', N, H * hd)
            n_const, kc_off, vc_off = 0, 0, 0
            if nuc_kv is not None:       # nuclear tokens: constant extra key / value rows (no derivative lanes)
                n_const = n_nuc
                kv_id = 2 * l * n_nuc * H * hd + np.arange(n_nuc * H * hd)       # derived vector: K_nuc then V_nuc of every layer
                kc_off = b.push_w(nuc_kv[l][0], ('', '', 'const', ()), derived=kv_id)
                vc_off = b.push_w(nuc_kv[l][1], ('', '', 'const', ()), derived=kv_id + n_nuc * H * hd)
            b.ops.append(Op(OP_ATTENTION, [q, k_, v, att, H, hd, n_const, kc_off, vc_off], note=f'layer {l} attention'))
            # attention FLOPs (QK^T and PV), algorithmic: 2 * 2 * N*(N + n_const)*D per walker
            b.flops += 4.0 * N * (N + n_const) * H * hd
            a2 = b.buf(f'l{l}/attended', N, x_dim)
            b.linear(f'{uf}/multi_head_attention/linear', [(att, 0, H * hd, 0)], a2, 0, 0, N, None, res=x, res_scale=1.0)
            xn = b.buf(f'x{l + 1}', N, x_dim)
            b.mlp(f'{uf}/mlp', spec.attn_mlp, [(a2, 0, x_dim, 0)], x_dim, x_dim, xn, 0, 0, N, N, res=a2, res_scale=1.0)
            x = xn
            continue
        pieces = []
        mean = -1
        cbuf, c_col = -1, 0
        n_conv = sum(1 for u in spec.update_features if u.startswith('conv_') or u.startswith('edge_'))
        c_width = sum(E if u.startswith('conv_') else e_dim for u in spec.update_features
                      if u.startswith('conv_') or u.startswith('edge_'))
        if n_conv:
            cbuf = b.buf(f'l{l}/agg', N, c_width)
        for uf in spec.update_features:
            if uf == 'residual':
                pieces.append((x, 0, x_dim, 0))
            elif uf in ('node_up', 'node_down'):
                if mean < 0:
                    mean = b.buf(f'l{l}/mean', 2, x_dim)     # the SPIN_MEAN op is emitted right before g
                pieces.append((mean, 0 if uf == 'node_up' else 1, x_dim, 1))
            elif uf.startswith('conv_'):
                t = uf[5:]
                base = f'{ln}/~/convolution_electron_update_feature/~single_edge_type_update'
                r0, nr = seg[t]
                we = b.names.get(f'l{l}/we')
                if we is None:
                    we = b.buf(f'l{l}/we', n_edge_rows, E)
                hx = b.buf(f'l{l}/hx_{t}', N, E)
                b.lockstep(
                    b.mlp_steps(f'{base}/w_{t}', spec.w, [(e, r0, e_dim, 0)], e_dim, E, we, r0, 0, nr, n_edge_rows),
                    b.mlp_steps(f'{base}/h_{t}', spec.h, [(x, 0, x_dim, 0)], x_dim, E, hx, 0, 0, N, N))
                tab, S = conv_tab[t]
                b.ops.append(Op(OP_CONV, [we, hx, cbuf, c_col, tab, S, E], note=f'layer {l} conv_{t}'))
                c_col += E
            elif uf.startswith('edge_'):
                t = uf[5:]
                tab, S = conv_tab[t]
                n_send = n_up if t == 'up' else n_down
                b.ops.append(Op(OP_EDGE_SUM, [e, max(n_send, 1), cbuf, c_col, tab, S, e_dim], [0, 0, 0, 0],
                                note=f'layer {l} edge_{t} mean'))
                c_col += e_dim
            else:
                raise ValueError(uf)
        if cbuf >= 0:
            pieces.append((cbuf, 0, c_width, 0))
        assert sum(p[2] for p in pieces) == row['cat']
        if mean >= 0:
            b.ops.append(Op(OP_SPIN_MEAN, [x, mean, n_up], note=f'layer {l} spin means'))
        xn = b.buf(f'x{l + 1}', N, D)
        resid = spec.electron_residual_normalize is not None and x_dim == D
        b.mlp(f'{ln}/~/g', spec.g, pieces, row['cat'], D, xn, 0, 0, N, N,
              res=x if resid else -1, res_scale=(S2 if spec.electron_residual_normalize else 1.0) if resid else 1.0)
        if spec.deep_features and not row['last']:
            en = b.buf(f'e{l + 1}', n_edge_rows, E)
            resid_e = spec.two_particle_residual_normalize is not None and e_dim == E
            b.mlp(f'{ln}/~/u', spec.u, [(e, 0, e_dim, 0)], e_dim, E, en, 0, 0, n_edge_rows, n_edge_rows,
                  res=e if resid_e else -1,
                  res_scale=(S2 if spec.two_particle_residual_normalize else 1.0) if resid_e else 1.0)
            e, e_dim = en, E
        x, x_dim = xn, D

    # ---- heads ----
    jas = -1
    if spec.jastrow is not None:
        xs = b.buf('x_sum', 1, x_dim)
        b.ops.append(Op(OP_ROW_SUM, [x, xs], note='Jastrow: sum over electrons'))
        jas = b.buf('jastrow', 1, 1)
        b.mlp(f'{OMNI}/~/Jastrow/~/mlp', spec.jastrow, [(xs, 0, x_dim, 0)], x_dim, 1, jas, 0, 0, 1, 1)
    assert spec.full_determinant, 'only full determinants are compiled'
    bf = b.buf('backflow', N, K * N)
    b.mlp(f'{OMNI}/~/Backflow/~/mlp', spec.backflow, [(x, 0, x_dim, 0)], x_dim, K * N, bf, 0, 0, n_up, N)
    b.mlp(f'{OMNI}/~/Backflow_1/~/mlp', spec.backflow, [(x, n_up, x_dim, 0)], x_dim, K * N, bf, n_up, 0, n_down, N)
    n_env = 1
    if spec.envelope == 'simplified':
        # wf/env.py:110-226 with pi = 1 and orbital-independent exponents, expanded to the general
        # [K*N orbitals][n_nuc * n_env] table the ORBITALS kernel reads: zeta[(k,mu)][(nuc,e)] = zetas[nuc,k,e]
        n_env = spec.n_envelope_per_nucleus
        offs = [b.push_w(np.ones((K * N, n_nuc * n_env)), ('', '', 'const', ())) for _ in range(2)]
        for s, spin in enumerate(('up', 'down')):
            z = np.transpose(nuc_zetas[spin], (1, 0, 2)).reshape(K, 1, n_nuc * n_env)
            # (derived vector: after the K / V rows of every layer, zetas up then down, each [n_nuc][K][n_env])
            z_id = 2 * len(rows) * n_nuc * D + s * n_nuc * K * n_env + np.arange(n_nuc * K * n_env).reshape(n_nuc, K, n_env)
            z_id = np.transpose(z_id, (1, 0, 2)).reshape(K, 1, n_nuc * n_env)
            offs.append(b.push_w(np.broadcast_to(z, (K, N, n_nuc * n_env)), ('', '', 'const', ()),
                                 derived=np.broadcast_to(z_id, (K, N, n_nuc * n_env))))
    else:
        env = params[f'{WF}/~/exponential_envelopes']
        offs = [b.push_w(env[nm], (f'{WF}/~/exponential_envelopes', nm, 'raw', ())) for nm in
                ('pi_up', 'pi_down', 'zetas_up', 'zetas_down')]
    orb = b.buf('orbitals', K, N * N)
    b.ops.append(Op(OP_ORBITALS, [bf, orb] + offs + [n_env], note='Slater matrices = envelope * backflow'))
    b.ops.append(Op(OP_SLOGDET, [orb], note='slogdet + derivative traces'))
    cc_off = -1
    if spec.conf_coeff == 'linear':
        cc_off = b.push_w(params[f'{WF}/~/conf_coeff']['w'], (f'{WF}/~/conf_coeff', 'w', 'raw', ()))
    cusp_kind = {None: 0, 'deepqmc': 1, 'psiformer': 2}[spec.cusp]
    if spec.cusp is not None and spec.cusp_trainable_alpha:
        cm = params[f'{WF}/~/electronic_cusp_asymptotic']
        al_off = b.push_w(np.array([float(cm['same_alpha']), float(cm['anti_alpha'])]),
                          (f'{WF}/~/electronic_cusp_asymptotic', ('same_alpha', 'anti_alpha'), 'alphas', ()),
                          [b.ids(f'{WF}/~/electronic_cusp_asymptotic', nm).reshape(-1)[0] for nm in ('same_alpha', 'anti_alpha')])
    else:
        al_off = b.push_w(np.array([spec.cusp_alpha, spec.cusp_alpha]), ('', '', 'const', ()))
    b.ops.append(Op(OP_FINAL, [jas, cc_off, cusp_kind, al_off], [spec.cusp_same_scale, spec.cusp_anti_scale, 0, 0],
                    note='CI sum + cusp + Jastrow (+ potentials, E_loc)'))
    return b.finish(Program(spec, n_up, n_down, n_nuc, b.bufs, b.ops, np.concatenate(b.w), np.asarray(b.it, np.int32),
                            b.names, b.slots, b.flops))
