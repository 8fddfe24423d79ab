"""Copy the reference's parameter-gradient golden into a small fixture.

Run in the build container (needs /root/reference):  python tests/golden/make_grad_golden.py
Writes tests/golden/reference_grad_psi.npz: d log|psi| / d theta of the reference's test ansatz (tests/conf/ansatz.yaml,
init(PRNGKey(0)) parameters) at its canonical LiH walker, one array per parameter leaf, keyed 'module:leaf' as in the
reference's tests/test_wf/test_grad_psi.npz (data only; no reference source is copied).
"""
import os

import numpy as np

REF = '/root/reference/tests'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'reference_grad_psi.npz')


def main():
    d = np.load(f'{REF}/test_wf/test_grad_psi.npz')
    np.savez_compressed(OUT, **{k: np.asarray(d[k], np.float64) for k in d.files})
    print(f'wrote {OUT}: {len(d.files)} leaves')


if __name__ == '__main__':
    main()
