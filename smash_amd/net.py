"""The neural network of the ANN regionalisation: a mirror of the reference's smash.Net (smash/core/net.py) as far as the descriptor ->
parameter mapping uses it.  Same option names, defaults, initialisers and optimizer formulas; the forward pass and the weight gradient
run through the host C++ of libsmashx (smashx_ann_host_*, csrc/sx_ann.h), which computes in fp64 on fp32 inputs, rounds every output
once to fp32 and shares its bits with the kernels that evaluate the same network on the device (include/smashx_ann.h).  The
optimizers run here, in numpy fp64.  softplus, softmax and dropout layers can be declared, as in the reference, and are refused when
the network is evaluated."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ANN_LAYER

__all__ = ["Net"]

WB_INITIALIZER = ["uniform", "glorot_uniform", "he_uniform", "normal", "glorot_normal", "he_normal", "zeros"]
NET_OPTIMIZER = ["sgd", "adam", "adagrad", "rmsprop"]
LAYER_NAME = ["dense", "activation", "scale", "dropout"]
ACTIVATIONS = ("relu", "sigmoid", "selu", "elu", "softmax", "leaky_relu", "tanh", "softplus")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _check_unknown_options(what, unknown):
    if unknown:
        raise KeyError("Unknown %s options: '%s'" % (what, ", ".join(map(str, unknown))))


# ---- layers -----------------------------------------------------------------------------------------------------------------------------
class Layer:
    trainable = True
    input_shape = None

    def _set_input_shape(self, shape):
        self.input_shape = shape

    def layer_name(self):
        return self.__class__.__name__

    def n_params(self):
        return 0

    def output_shape(self):
        return self.input_shape


class Dense(Layer):
    def __init__(self, neurons, input_shape=None, kernel_initializer="glorot_uniform", bias_initializer="zeros", **unknown_options):
        _check_unknown_options("Dense Layer", unknown_options)
        self.input_shape = input_shape
        self.neurons = neurons
        self.trainable = True
        self.weight = None
        self.bias = None
        self.kernel_initializer = kernel_initializer.lower()
        if self.kernel_initializer not in WB_INITIALIZER:
            raise ValueError(f"Unknown kernel initializer: {self.kernel_initializer}. Choices {WB_INITIALIZER}")
        self.bias_initializer = bias_initializer.lower()
        if self.bias_initializer not in WB_INITIALIZER:
            raise ValueError(f"Unknown bias initializer: {self.bias_initializer}. Choices {WB_INITIALIZER}")

    def _initialize(self, optimizer):
        self.weight = _wb_initialization(self, "weight")
        self.bias = _wb_initialization(self, "bias")
        self._weight_opt = copy.copy(optimizer)
        self._bias_opt = copy.copy(optimizer)

    def n_params(self):
        return int(np.prod(self.weight.shape) + np.prod(self.bias.shape))

    def output_shape(self):
        return (self.neurons,)


class Activation(Layer):
    def __init__(self, name, **unknown_options):
        _check_unknown_options("Activation Layer", unknown_options)
        if name.lower() not in ACTIVATIONS:
            raise KeyError(name.lower())
        self.activation_name = name

    def layer_name(self):
        return "Activation (%s)" % self.activation_name


class Scale(Layer):
    def __init__(self, bounds, **unknown_options):
        _check_unknown_options("Scale Layer", unknown_options)
        self.scale_name = "minmaxscale"
        self._bounds = np.array(bounds)
        self.lower = np.array([b[0] for b in self._bounds], np.float64)
        self.upper = np.array([b[1] for b in self._bounds], np.float64)

    def layer_name(self):
        return "Scale (MinMaxScale)"


class Dropout(Layer):
    def __init__(self, drop_rate, **unknown_options):
        _check_unknown_options("Dropout Layer", unknown_options)
        self.drop_rate = drop_rate


LAYERS = {"dense": Dense, "activation": Activation, "scale": Scale, "dropout": Dropout}


def _wb_initialization(layer, attr):
    """net.py:537-576: the draws of the reference, in its order (np.random's global state, seeded by compile)"""
    fin, fout = layer.input_shape[0], layer.neurons
    initializer, shape = (layer.bias_initializer, (1, fout)) if attr == "bias" else (layer.kernel_initializer, (fin, fout))
    split = initializer.split("_")
    if split[-1] == "uniform":
        limit = np.sqrt(6 / (fin + fout)) if split[0] == "glorot" else np.sqrt(6 / fin) if split[0] == "he" else 1 / np.sqrt(fin)
        return np.random.uniform(-limit, limit, shape)
    if split[-1] == "normal":
        std = np.sqrt(2 / (fin + fout)) if split[0] == "glorot" else np.sqrt(2 / fin) if split[0] == "he" else 0.01
        return np.random.normal(0, std, shape)
    return np.zeros(shape)


# ---- optimizers (net.py:848-999) ----------------------------------------------------------------------------------------------------------
class StochasticGradientDescent:
    def __init__(self, learning_rate=0.01, momentum=0, **unknown_options):
        _check_unknown_options("SGD optimizer", unknown_options)
        self.learning_rate, self.momentum, self.w_updt = learning_rate, momentum, None

    def update(self, w, grad_wrt_w):
        if self.w_updt is None:
            self.w_updt = np.zeros(np.shape(w))
        self.w_updt = self.momentum * self.w_updt + (1 - self.momentum) * grad_wrt_w
        return w - self.learning_rate * self.w_updt


class Adam:
    def __init__(self, learning_rate=0.001, b1=0.9, b2=0.999, **unknown_options):
        _check_unknown_options("Adam optimizer", unknown_options)
        self.learning_rate, self.eps, self.m, self.v, self.b1, self.b2 = learning_rate, 1e-8, None, None, b1, b2

    def update(self, w, grad_wrt_w):
        if self.m is None:
            self.m = np.zeros(np.shape(grad_wrt_w))
            self.v = np.zeros(np.shape(grad_wrt_w))
        self.m = self.b1 * self.m + (1 - self.b1) * grad_wrt_w
        self.v = self.b2 * self.v + (1 - self.b2) * np.power(grad_wrt_w, 2)
        m_hat = self.m / (1 - self.b1)          # the reference divides by 1 - b, not by 1 - b ** t
        v_hat = self.v / (1 - self.b2)
        self.w_updt = self.learning_rate * m_hat / (np.sqrt(v_hat) + self.eps)
        return w - self.w_updt


class Adagrad:
    def __init__(self, learning_rate=0.01, **unknown_options):
        _check_unknown_options("Adagrad optimizer", unknown_options)
        self.learning_rate, self.G, self.eps = learning_rate, None, 1e-8

    def update(self, w, grad_wrt_w):
        if self.G is None:
            self.G = np.zeros(np.shape(w))
        self.G = self.G + np.power(grad_wrt_w, 2)
        return w - self.learning_rate * grad_wrt_w / np.sqrt(self.G + self.eps)


class RMSprop:
    def __init__(self, learning_rate=0.001, rho=0.9, **unknown_options):
        _check_unknown_options("RMSprop optimizer", unknown_options)
        self.learning_rate, self.Eg, self.eps, self.rho = learning_rate, None, 1e-8, rho

    def update(self, w, grad_wrt_w):
        if self.Eg is None:
            self.Eg = np.zeros(np.shape(grad_wrt_w))
        self.Eg = self.rho * self.Eg + (1 - self.rho) * np.power(grad_wrt_w, 2)
        return w - self.learning_rate * grad_wrt_w / np.sqrt(self.Eg + self.eps)


OPT_FUNC = {"sgd": StochasticGradientDescent, "adam": Adam, "adagrad": Adagrad, "rmsprop": RMSprop}


# ---- the network --------------------------------------------------------------------------------------------------------------------------
class Net:
    """smash.Net: add(layer, options), compile(optimizer, options, random_state), copy(), set_trainable(trainable), layers, history."""

    def __init__(self):
        self.layers = []
        self.history = {"loss_train": [], "loss_valid": []}
        self._optimizer = None
        self._learning_rate = None
        self._compiled = False

    def __repr__(self):
        if not (self._compiled and self.layers):
            return "The network does not contain layers or has not been compiled yet"
        rows = [(l.layer_name(), f"{l.input_shape}/{l.output_shape()}", l.n_params(), l.trainable) for l in self.layers]
        ret = [f"{n:24s}{s:24s}{p}" for n, s, p, _ in rows]
        ret.append(f"Total parameters: {sum(r[2] for r in rows)}")
        ret.append(f"Trainable parameters: {sum(r[2] for r in rows if r[3])}")
        ret.append(f"Optimizer: ({self._optimizer}, lr={self._learning_rate})")
        return "\n".join(ret)

    def add(self, layer, options):
        if not isinstance(layer, str):
            raise TypeError("layer argument must be str")
        layer = layer.lower()
        if layer not in LAYER_NAME:
            raise ValueError(f"Unknown layer type '{layer}'. Choices: {LAYER_NAME}")
        lay = LAYERS[layer](**options)
        if not self.layers:
            if "input_shape" not in options:
                raise TypeError("First layer missing required option argument: 'input_shape'")
            if not isinstance(options["input_shape"], tuple):
                raise ValueError(f"input_shape option should be a tuple, not {type(options['input_shape'])}")
        else:
            lay._set_input_shape(shape=self.layers[-1].output_shape())
        self.layers.append(lay)

    def compile(self, optimizer="adam", options=None, random_state=None):
        if not self.layers:
            raise ValueError("The network does not contain layers")
        if not isinstance(optimizer, str):
            raise TypeError("optimizer argument must be str")
        optimizer = optimizer.lower()
        if optimizer not in NET_OPTIMIZER:
            raise ValueError(f"Unknown optimizer '{optimizer}'. Choices: {NET_OPTIMIZER}")
        if random_state is not None:
            np.random.seed(random_state)
        opt = OPT_FUNC[optimizer](**(options or {}))
        for layer in self.layers:
            if hasattr(layer, "_initialize"):
                layer._initialize(opt)
        self._compiled = True
        self._optimizer = optimizer
        self._learning_rate = opt.learning_rate

    def copy(self):
        return copy.deepcopy(self)

    def set_trainable(self, trainable):
        if len(trainable) != len(self.layers):
            raise ValueError(f"Inconsistent length between trainable ({len(trainable)}) and the number of layers ({len(self.layers)})")
        for layer, t in zip(self.layers, trainable):
            layer.trainable = t

    # -- the graph and the packed weights as libsmashx takes them (include/smashx_ann.h) --------------------------------------------
    def _dense(self):
        return [l for l in self.layers if isinstance(l, Dense)]

    def graph(self):
        """(nd, kind int32[nlayers], width int32[nlayers], ncv, lower float64[ncv] | None, upper | None)"""
        if not self.layers:
            raise ValueError("The graph has not been set yet")
        kind, width, lower, upper = [], [], None, None
        for l in self.layers:
            if isinstance(l, Dense):
                kind.append(ANN_LAYER["dense"])
            elif isinstance(l, Activation):
                kind.append(ANN_LAYER[l.activation_name.lower()])
            elif isinstance(l, Scale):
                kind.append(ANN_LAYER["scale"])
                lower, upper = np.ascontiguousarray(l.lower, np.float64), np.ascontiguousarray(l.upper, np.float64)
            else:
                kind.append(ANN_LAYER["dropout"])
            width.append(int(l.output_shape()[0]))
        return int(self.layers[0].input_shape[0]), np.array(kind, np.int32), np.array(width, np.int32), width[-1], lower, upper

    def _graph_args(self):
        nd, kind, width, ncv, lower, upper = self.graph()
        if lower is not None and lower.size != ncv:
            raise _lib.SmashxError(_lib.E_ARG, f"the scale layer has {lower.size} bounds, the network {ncv} outputs")
        return (nd, len(kind), _ptr(kind), _ptr(width), ncv), (_ptr(lower), _ptr(upper)), (kind, width, lower, upper)

    def weights(self):
        """the packed weights, float64: per dense layer W (fin, fout) in C order, then b"""
        if not self._compiled:
            raise ValueError("The network has not been compiled yet")
        return np.concatenate([np.concatenate([np.asarray(l.weight, np.float64).ravel(), np.asarray(l.bias, np.float64).ravel()])
                               for l in self._dense()])

    def set_weights(self, w):
        k = 0
        for l in self._dense():
            fin, fout = l.input_shape[0], l.neurons
            l.weight = np.array(w[k:k + fin * fout], np.float64).reshape(fin, fout)
            l.bias = np.array(w[k + fin * fout:k + (fin + 1) * fout], np.float64).reshape(1, fout)
            k += (fin + 1) * fout

    def _forward_pass(self, x_train, training=True):
        """y (n, ncv) float32: the network at the rows of x (n, nd) float32"""
        g, b, keep = self._graph_args()
        x = np.ascontiguousarray(x_train, np.float32)
        if x.ndim != 2 or x.shape[1] != g[0]:
            raise _lib.SmashxError(_lib.E_ARG, f"x must be (n, {g[0]})")
        w = self.weights()
        y = np.zeros((x.shape[0], g[4]), np.float32)
        _lib.check(_lib.lib().smashx_ann_host_forward(*g, *b, _ptr(w), x.shape[0], _ptr(x), _ptr(y)))
        return y

    _predict = _forward_pass

    def gradient(self, x_train, loss_grad):
        """the packed gradient w.r.t. the weights of sum(loss_grad * y) -- rows in the order of the sums (csrc/sx_ann.h)"""
        g, b, keep = self._graph_args()
        x = np.ascontiguousarray(x_train, np.float32)
        lg = np.ascontiguousarray(loss_grad, np.float32)
        if x.ndim != 2 or x.shape[1] != g[0] or lg.shape != (x.shape[0], g[4]):
            raise _lib.SmashxError(_lib.E_ARG, f"x must be (n, {g[0]}) and loss_grad (n, {g[4]})")
        w = self.weights()
        wb = np.zeros_like(w)
        _lib.check(_lib.lib().smashx_ann_host_gradient(*g, *b, _ptr(w), x.shape[0], _ptr(x), _ptr(lg), _ptr(wb)))
        return wb

    def update(self, weights_b):
        """Dense._backward_pass's update (net.py:669-680) with a packed gradient: the layers last to first, weight before bias; a
        layer that is not trainable keeps its weights"""
        offs, k = [], 0
        for l in self._dense():
            offs.append(k)
            k += (l.input_shape[0] + 1) * l.neurons
        for l, k in reversed(list(zip(self._dense(), offs))):
            if not l.trainable:
                continue
            fin, fout = l.input_shape[0], l.neurons
            l.weight = l._weight_opt.update(l.weight, np.asarray(weights_b[k:k + fin * fout]).reshape(fin, fout))
            l.bias = l._bias_opt.update(l.bias, np.asarray(weights_b[k + fin * fout:k + (fin + 1) * fout]).reshape(1, fout))

    def _backward_pass(self, loss_grad, x_train):
        self.update(self.gradient(x_train, loss_grad))
