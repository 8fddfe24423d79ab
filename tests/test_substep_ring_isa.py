"""The ring barrier of the generated sub-step kernel (spec_device.h ring_barrier<K>: `s_waitcnt lgkmcnt(K); s_barrier`) is only
safe if the wave's last ring store (ds_write) has landed when the barrier passes.  LDS operations complete in order, so that
holds when at least K ds_read follow the last ds_write before the barrier IN THE COMPILED CODE -- the generator counts them in
source order, the compiler may reorder.  Compiles the committed deepqmc_amd/csrc/gen/substep_lih_paulinet.hip with the
Makefile's flags (device code only, ~5 s) and checks every `s_waitcnt lgkmcnt(K)` + `s_barrier` of both instances."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'deepqmc_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def _cxxflags():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS\s*=\s*(.*)$', mk, re.M).group(1)
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', mk, re.M).group(1)
    return flags.replace('$(ARCH)', arch).split()


def ring_barriers(asm, instance):
    """[(K, ds_read since the last ds_write)] for every `s_waitcnt ... lgkmcnt(K)` directly followed by `s_barrier`"""
    lines = asm.split('\n')
    start = next(i for i, l in enumerate(lines) if re.match(r'^_Z\S*k_substep_\S*' + instance + r'\S*:', l))
    reads, prev, out = 0, '', []
    for l in lines[start + 1:]:
        l = l.split(';')[0].strip()
        if not l or l.endswith(':') or l.startswith('.'):
            continue
        op = l.split()[0]
        if op == 's_endpgm':
            break
        if op.startswith('ds_write'):
            reads = 0
        elif op.startswith('ds_read'):
            reads += 1
        elif op == 's_barrier':
            m = re.match(r's_waitcnt\b.*\blgkmcnt\((\d+)\)', prev)
            if m:
                out.append((int(m.group(1)), reads))
        prev = l
    return out


def test_ring_barriers_wait_for_the_last_ring_store(tmp_path):
    if not os.path.exists(HIPCC) and shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which('hipcc')
    out = tmp_path / 'substep.s'
    subprocess.run([hipcc, *_cxxflags(), '--cuda-device-only', '-S', 'gen/substep_lih_paulinet.hip', '-o', str(out)],
                   cwd=CSRC, check=True)
    asm = out.read_text()
    for instance in ('ILb0E', 'ILb1E'):
        bars = ring_barriers(asm, instance)
        assert sum(1 for k, _ in bars if k > 0) > 0, f'{instance}: no ring barrier found'
        bad = [(i, k, r) for i, (k, r) in enumerate(bars) if k > r]
        assert not bad, f'{instance}: (barrier #, lgkmcnt K, ds_read after the last ds_write) with K > reads: {bad}'
