"""Float64 restatement of the three Keras 2.1 optimizer updates the package launches (keras/optimizers.py: Adam with and without
amsgrad, SGD with momentum / nesterov), of get_gradients' clipping and of the joint model's regularised gradient.  A plain module
(`import _optimizer_ref as R`), NumPy only; tests/test_optimizer_args.py holds it to closed forms, tests/test_gpu_optimizers.py holds
the kernels and the models to it.

t is 1-based (t = iterations + 1: `t - 1` updates are complete), lr_d = lr / (1 + decay * (t - 1))."""
import numpy as np


def lr_decayed(lr, decay, t):
    return lr / (1.0 + decay * (t - 1))


def adam_word(t, lr=1e-3, b1=0.9, b2=0.999, decay=0.0):
    """Keras' lr_t of update t."""
    return lr_decayed(lr, decay, t) * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def regularised(g, p, coef, mask=None):
    """g * mask + 2 * coef * p: the gradient of loss + sum coef * p^2 over the trainable subset."""
    g, p = np.asarray(g, np.float64), np.asarray(p, np.float64)
    return g * (1.0 if mask is None else np.asarray(mask, np.float64)) + 2.0 * np.asarray(coef, np.float64) * p


def clipped(g, grad_scale=1.0, clipnorm=None, clipvalue=None):
    """get_gradients: the scaled gradient clipped by its global norm (g * clipnorm / norm when norm >= clipnorm), then by value."""
    g = np.asarray(g, np.float64) * grad_scale
    if clipnorm:
        norm = np.sqrt((g * g).sum())
        if norm >= clipnorm:
            g = g * (clipnorm / norm)
    if clipvalue:
        g = np.clip(g, -clipvalue, clipvalue)
    return g


def adam_step(p, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, decay=0.0):
    """-> (p, m, v)"""
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return p - adam_word(t, lr, b1, b2, decay) * m / (np.sqrt(v) + eps), m, v


def amsgrad_step(p, g, m, v, vhat, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, decay=0.0):
    """-> (p, m, v, vhat)"""
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    vhat = np.maximum(vhat, v)
    return p - adam_word(t, lr, b1, b2, decay) * m / (np.sqrt(vhat) + eps), m, v, vhat


def sgd_step(p, g, vel, t, lr=0.01, momentum=0.0, nesterov=False, decay=0.0):
    """-> (p, velocity): v = momentum * m - lr_d * g; m := v; p += momentum * v - lr_d * g if nesterov else v."""
    u = lr_decayed(lr, decay, t) * g
    vel = momentum * vel - u
    return p + (momentum * vel - u if nesterov else vel), vel


class Trajectory(object):
    """One optimizer's state over a flat float64 parameter vector: step(g) applies update t = 1, 2, ... to self.p.
    kind: "adam" | "amsgrad" | "sgd"; kw: the step function's keywords (lr, decay, b1 / b2 / eps or momentum / nesterov)."""

    def __init__(self, kind, p, clipnorm=None, clipvalue=None, **kw):
        self.kind, self.p, self.kw = kind, np.array(p, np.float64), kw
        self.clipnorm, self.clipvalue = clipnorm, clipvalue
        self.state = [np.zeros_like(self.p) for _ in range({"adam": 2, "amsgrad": 3, "sgd": 1}[kind])]
        self.t = 0

    def step(self, g, grad_scale=1.0):
        self.t += 1
        g = clipped(g, grad_scale, self.clipnorm, self.clipvalue)
        fn = {"adam": adam_step, "amsgrad": amsgrad_step, "sgd": sgd_step}[self.kind]
        out = fn(self.p, g, *self.state, self.t, **self.kw)
        self.p, self.state = out[0], list(out[1:])
        return self.p
