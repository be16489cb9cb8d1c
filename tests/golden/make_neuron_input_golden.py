#!/usr/bin/env python3
"""Capture the fixture of tests/test_neuron_input.py::test_reference_working_memory_class_on_our_stack from a checkout of the
reference (sspslam).

The reference's OWN ``AdditiveInputGatedMemory`` (``sspslam/networks/workingmemory.py``) is loaded with zero edits and this repo's
object model registered as ``import nengo``, wired as the test wires ours and built by our builder; the census of its objects,
its operator list and its buffers go to ``neuron_input_dropin.npz``.  This repo's class is built beside it and must give the
same.  Nothing from the reference's source is copied: the fixture holds what was built only.

    python tests/golden/make_neuron_input_golden.py PATH_TO_REFERENCE_CHECKOUT
"""
import importlib.util
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(ref):
    import sspslam_amd.frontend as fe
    from sspslam_amd.builder import build
    from sspslam_amd.networks import AdditiveInputGatedMemory
    from test_neuron_input import census, gated_memory
    fe.install_as_nengo(force=True)
    spec = importlib.util.spec_from_file_location("_reference_workingmemory",
                                                  os.path.join(ref, "sspslam", "networks", "workingmemory.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    theirs = gated_memory(mod.AdditiveInputGatedMemory, fe.EnsembleArray)
    ours = gated_memory(AdditiveInputGatedMemory, fe.EnsembleArray)
    assert census(theirs) == census(ours)
    a, b = build(theirs), build(ours)
    assert [o["kind"] for o in a.ops] == [o["kind"] for o in b.ops] and a.sig_size == b.sig_size and len(a.buffers) == len(b.buffers)
    for x, y in zip(a.buffers, b.buffers):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    n_nodes, n_ens, n_conn, nodes = census(theirs)
    g = {"census": np.array([n_nodes, n_ens, n_conn]), "node_labels": np.array([lb for lb, _ in nodes]),
         "node_size_in": np.array([sz for _, sz in nodes]), "op_kinds": np.array([o["kind"] for o in a.ops]),
         "sig_size": np.array(a.sig_size), "n_buffers": np.array(len(a.buffers))}
    for i, x in enumerate(a.buffers):
        g[f"buffer_{i}"] = np.asarray(x)
    fn = os.path.join(OUT, "neuron_input_dropin.npz")
    np.savez_compressed(fn, **g)
    print(f"  {os.path.basename(fn)} {os.path.getsize(fn) / 1024:.1f} KiB")


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "sspslam")):
        sys.exit(__doc__)
    main(sys.argv[1])
