"""Object construction by dotted path -- the plugin mechanism of the reference
(utils/train_util.py:120-137): ``{"type": "pkg.mod.Class", "args": {...}}`` with nested dicts
instantiated recursively -- and the reference's mixup helpers (utils/train_util.py:48-88), where a
reference-style training runner looks for them."""
import importlib

import numpy as np
import torch


def get_obj_from_str(string):
    module, cls = string.rsplit(".", 1)
    return getattr(importlib.import_module(module), cls)


def init_obj_from_str(config, **kwargs):
    args = dict(config.get("args", {}))
    args.update(kwargs)
    for k, v in config.items():
        if k not in ("type", "args") and isinstance(v, dict) and k not in kwargs:
            args[k] = init_obj_from_str(v)
    return get_obj_from_str(config["type"])(**args)


class Mixup(object):
    """Mixup coefficient generator: per clip pair (2k, 2k+1), lambda ~ Beta(alpha, alpha) and 1 - lambda, from a numpy
    RandomState of its own (utils/train_util.py:48-70)."""

    def __init__(self, mixup_alpha, random_seed=1234):
        self.mixup_alpha = mixup_alpha
        self.random_state = np.random.RandomState(random_seed)

    def get_lambda(self, batch_size):
        """(batch_size,) float64 numpy array [l0, 1 - l0, l1, 1 - l1, ...]."""
        mixup_lambdas = []
        for _ in range(0, batch_size, 2):
            lam = self.random_state.beta(self.mixup_alpha, self.mixup_alpha, 1)[0]
            mixup_lambdas.append(lam)
            mixup_lambdas.append(1. - lam)
        return np.array(mixup_lambdas)


def do_mixup(x, mixup_lambdas):
    """out[k] = x[2k] * lambda[2k] + x[2k+1] * lambda[2k+1] along dim 0 (utils/train_util.py:73-88): lambda taken as given, in
    fp32; (2N, ...) -> (N, ...).  The encoder applies the same to its bn0 output in csrc/augment.hip; here it serves small
    tensors such as the frame lengths."""
    mixup_lambdas = torch.as_tensor(mixup_lambdas, dtype=torch.float).to(x.device)
    return (x[0::2].transpose(0, -1) * mixup_lambdas[0::2] +
            x[1::2].transpose(0, -1) * mixup_lambdas[1::2]).transpose(0, -1)
