"""Writes tests/golden/golden_minres_rules.npz: what lzh_minres_start and lzh_minres_scalars of the
built liblz_host.so return on test_minres_host.rule_grid() (special values of every dot).
Regenerate it only from a library whose rules are meant to be the new truth.

    python tests/golden/make_golden_minres.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if __name__ == "__main__":
    import __graft_entry__ as ge
    from test_minres_host import rule_outputs
    out = rule_outputs(ge.load_package())
    np.savez_compressed(os.path.join(HERE, "golden_minres_rules.npz"), **out)
    print("wrote", os.path.join(HERE, "golden_minres_rules.npz"), len(out), "arrays")
