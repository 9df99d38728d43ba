"""Plain-torch restatement of the MuonWithAuxAdam specification (the `muon` package the reference's scripts/train.py:262-307
imports is not part of the reference tree).  float64 is the yardstick; bfloat16 and float32 measure how far those number
formats alone are from it.

Muon group, per parameter p with gradient g, state momentum_buffer m (zeros at first use), lr, momentum beta, weight_decay:

    m  <- m + (1-beta)*(g - m)
    u  <- g + beta*(m - g)                                  (Nesterov)
    U  <- u viewed as (shape[0], numel/shape[0])
    X  <- U (transposed if rows > cols);  X <- X / (||X||_F + 1e-7)
    5 times:  A = X X^T;  B = b*A + c*A*A;  X = a*X + B*X   (a, b, c) = (3.4445, -4.7750, 2.0315)
    O  <- X (transposed back)
    p  <- p*(1 - lr*weight_decay) - lr*sqrt(max(1, p.shape[-2]/p.shape[-1]))*O

Auxiliary group: Adam with bias correction and decoupled weight decay.
"""
import torch

NS_COEFFS = (3.4445, -4.7750, 2.0315)
NS_STEPS = 5
MUON_DEFAULTS = dict(lr=0.02, momentum=0.95, weight_decay=0.0)
ADAM_DEFAULTS = dict(lr=3e-4, betas=(0.9, 0.95), eps=1e-10, weight_decay=0.0)


def newton_schulz(U, dtype=torch.float64, steps=NS_STEPS):
    """U: (rows, cols) matrix or a batch of them -> the orthogonalised matrix, computed and returned in `dtype`"""
    a, b, c = NS_COEFFS
    X = U.to(dtype)
    transposed = X.size(-2) > X.size(-1)
    if transposed:
        X = X.mT
    X = X / (X.norm(dim=(-2, -1), keepdim=True) + 1e-7)
    for _ in range(steps):
        A = X @ X.mT
        B = b * A + c * (A @ A)
        X = a * X + B @ X
    if transposed:
        X = X.mT
    return X


def muon_scale(shape):
    return max(1.0, shape[-2] / shape[-1]) ** 0.5


def muon_update(p, g, m, lr, beta, weight_decay, ns_dtype=None):
    """one Muon step on p (in place) with gradient g and momentum buffer m (in place), in p's dtype; the Newton-Schulz
    iteration runs in ns_dtype (default: p's dtype)"""
    m.lerp_(g, 1 - beta)
    u = g.lerp(m, beta)
    O = newton_schulz(u.reshape(u.shape[0], -1), ns_dtype or p.dtype).to(p.dtype).reshape(p.shape)
    p.mul_(1 - lr * weight_decay).add_(O, alpha=-lr * muon_scale(p.shape))


def adam_update(p, g, exp_avg, exp_avg_sq, step, lr, betas, eps, weight_decay):
    """one auxiliary Adam step (bias correction, decoupled weight decay), in place; `step` counts from 1"""
    b1, b2 = betas
    exp_avg.lerp_(g, 1 - b1)
    exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
    m_hat = exp_avg / (1 - b1 ** step)
    v_hat = exp_avg_sq / (1 - b2 ** step)
    p.mul_(1 - lr * weight_decay)
    p.add_(m_hat / (v_hat.sqrt() + eps), alpha=-lr)


class RefMuonWithAuxAdam(torch.optim.Optimizer):
    """the specification as a torch optimizer over parameters of any float dtype, on any device; ns_dtype: the dtype of the
    Newton-Schulz iteration (None: the parameter's own)"""

    def __init__(self, param_groups, ns_dtype=None):
        groups = []
        for g in param_groups:
            if "use_muon" not in g:
                raise ValueError("every param group needs use_muon")
            g = dict(g)
            g["params"] = list(g["params"])
            for k, v in (MUON_DEFAULTS if g["use_muon"] else ADAM_DEFAULTS).items():
                g.setdefault(k, v)
            if g["use_muon"] and any(p.ndim < 2 for p in g["params"]):
                raise ValueError("a use_muon group holds a parameter with ndim < 2")
            groups.append(g)
        super().__init__(groups, dict())
        self.ns_dtype = ns_dtype

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if group["use_muon"]:
                    if not st:
                        st["momentum_buffer"] = torch.zeros_like(p)
                    muon_update(p, p.grad, st["momentum_buffer"], group["lr"], group["momentum"], group["weight_decay"],
                                self.ns_dtype)
                else:
                    if not st:
                        st["step"] = 0
                        st["exp_avg"] = torch.zeros_like(p)
                        st["exp_avg_sq"] = torch.zeros_like(p)
                    st["step"] += 1
                    adam_update(p, p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"], group["lr"], group["betas"],
                                group["eps"], group["weight_decay"])
