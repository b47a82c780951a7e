"""Shared by tests/test_ann_cpu.py and tests/test_gpu_ann.py: the fixtures of tests/golden/ann/ (tests/golden/make_ann.py), networks
built from a short specification, and the comparison of fp64 / fp32 arrays by their bits."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))

import golden_util as gu  # noqa: E402

DIR = os.path.join(gu.GOLDEN_DIR, "ann")
ACTIVATIONS = ("relu", "leaky_relu", "elu", "selu", "sigmoid", "tanh")
OPTIMIZERS = ("sgd", "adam", "adagrad", "rmsprop")
# the recorded trainings: name -> (net specification or None for the auto-graph, optimizer, options, epochs, early_stopping)
FIT_CASES = {
    "auto_adam_1": (None, "adam", {"learning_rate": 0.003}, 1, False),
    "auto_adam_4": (None, "adam", {"learning_rate": 0.003}, 4, False),
    "auto_adam_4_early": (None, "adam", {"learning_rate": 0.003}, 4, True),
    "tanh_elu_sgd_4": ([(6, "tanh"), (5, "elu"), (None, "sigmoid"), "scale"], "sgd", {"learning_rate": 0.05, "momentum": 0.5}, 4, False),
}
FIT_CONTROL = ("cp", "cft", "exc", "lr")
FIT_BOUNDS = ((1.0, 1000.0), (1.0, 1000.0), (-20.0, 5.0), (1.0, 200.0))
FIT_SEED = 11


def fixture(name):
    return np.load(os.path.join(DIR, name + ".npz"))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(a.view(u), b.view(u))


def build_net(Net, nd, spec, ncv, bounds=None, optimizer="adam", options=None, random_state=5, bias="normal"):
    """spec: a list of (neurons or None for ncv, activation name | tuple of names | None) per dense layer, and "scale".  Biases are
    drawn (not zero) unless bias = "zeros", so that every weight matters in a comparison."""
    net = Net()
    first = True
    for item in spec:
        if item == "scale":
            net.add("scale", {"bounds": bounds})
            continue
        neurons, acts = item
        opt = {"neurons": ncv if neurons is None else neurons, "bias_initializer": bias}
        if first:
            opt["input_shape"] = (nd,)
            first = False
        net.add("dense", opt)
        for a in (acts,) if isinstance(acts, str) else (acts or ()):
            net.add("activation", {"name": a})
    net.compile(optimizer, options or {}, random_state)
    return net


def column_major_cells(active_cell):
    """(rows, cols) of the active cells in column-major order, (rows, cols) of the others"""
    act = np.asarray(active_cell) == 1
    cc, rr = np.nonzero(act.T)
    ci, ri = np.nonzero(~act.T)
    return (rr, cc), (ri, ci)
