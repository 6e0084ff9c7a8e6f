"""Optimisers for embedding tables with sparse gradients - SparseSGD (with momentum),
SparseAdagrad and SparseAdam: the four the reference offers every model
(tf_euler/python/utils/optimizers.py: sgd, momentum, adagrad, adam), each step ONE fused call of
ops.sparse_row_step per parameter.

step() takes every parameter whose .grad is a sparse COO tensor with one sparse and one dense
dimension - what skipgram_loss, triple_score & co. return with sparse_grad=True and what
nn.Embedding(sparse=True) produces - and hands grad._indices()[0] and grad._values() to the kernel
WITHOUT coalescing: a coalesced and an uncoalesced gradient are both lists of occurrences, and
the kernel sums the occurrences of a row in their order.  Only rows the gradient names move
(lazy semantics), in the parameter and in its state.  A parameter without a gradient is skipped;
a dense gradient raises, as torch.optim.SparseAdam does.

The state keys are those of torch's own optimisers (step, exp_avg, exp_avg_sq, sum,
momentum_buffer), so a state_dict() of SparseAdam loads into torch.optim.SparseAdam and back.
The state tensors are fp32 whatever the table's dtype, and load_state_dict keeps them fp32.
Weight decay, Nesterov, amsgrad, lr_decay and maximize are not offered."""
import torch

from . import ops


def _occurrences(name, p):
    """(ids [nnz], rows [nnz, d]) of p.grad, uncoalesced as it is"""
    g = p.grad
    if not g.is_sparse:
        raise RuntimeError("%s does not support dense gradients, please consider a dense optimizer instead" % name)
    if p.dim() != 2 or g.sparse_dim() != 1 or g.dense_dim() != 1:
        raise RuntimeError("%s: a parameter is a [rows, d] table and its gradient a sparse COO tensor with one "
                           "sparse and one dense dimension" % name)
    return g._indices()[0], g._values()


class _SparseRowOptimizer(torch.optim.Optimizer):
    def _state_of(self, p, group):
        raise NotImplementedError

    def _row_step(self, p, ids, rows, state, group):
        raise NotImplementedError

    def load_state_dict(self, state_dict):
        """torch's load_state_dict casts every floating-point state tensor to its parameter's dtype;
        the state of a bf16 / fp16 table is fp32 and stays so: the saved tensors are put back as
        fp32 on the parameter's device, so a checkpoint resumes with the bits it was saved with"""
        super().load_state_dict(state_dict)
        saved_ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(saved_ids, params):
            for key, value in state_dict["state"].get(i, {}).items():
                if torch.is_tensor(value) and value.is_floating_point():
                    self.state[p][key] = value.detach().to(device=p.device, dtype=torch.float32, copy=True)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = type(self).__name__
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                ids, rows = _occurrences(name, p)
                self._row_step(p, ids, rows, self._state_of(p, group), group)
        return loss


def _need(cond, what):
    if not cond:
        raise ValueError("Invalid " + what)


class SparseSGD(_SparseRowOptimizer):
    """p -= lr * g, or with momentum > 0 TensorFlow's SparseApplyMomentum: a = momentum * a + g,
    p -= lr * a on the rows the gradient names (the other rows and their accumulators rest)."""

    def __init__(self, params, lr, momentum=0.0):
        _need(lr >= 0.0, "learning rate: %r" % (lr,))
        _need(momentum >= 0.0, "momentum value: %r" % (momentum,))
        super().__init__(params, dict(lr=lr, momentum=momentum))

    def _state_of(self, p, group):
        state = self.state[p]
        if group["momentum"] != 0 and "momentum_buffer" not in state:
            state["momentum_buffer"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
        return state

    def _row_step(self, p, ids, rows, state, group):
        if group["momentum"] != 0:
            ops.sparse_row_step("momentum", p, ids, rows, (state["momentum_buffer"],), lr=group["lr"],
                                momentum=group["momentum"])
        else:
            ops.sparse_row_step("sgd", p, ids, rows, lr=group["lr"])


class SparseAdagrad(_SparseRowOptimizer):
    """sum += g * g, p -= lr * g / (sqrt(sum) + eps) on the rows the gradient names: the sparse
    branch of torch.optim.Adagrad (eps = 0: TensorFlow's AdagradOptimizer)."""

    def __init__(self, params, lr, initial_accumulator_value=0.1, eps=1e-10):
        _need(lr >= 0.0, "learning rate: %r" % (lr,))
        _need(initial_accumulator_value >= 0.0, "initial_accumulator_value value: %r" % (initial_accumulator_value,))
        _need(eps >= 0.0, "epsilon value: %r" % (eps,))
        super().__init__(params, dict(lr=lr, initial_accumulator_value=initial_accumulator_value, eps=eps))

    def _state_of(self, p, group):
        state = self.state[p]
        if "sum" not in state:
            state["step"] = 0
            state["sum"] = torch.full(p.shape, float(group["initial_accumulator_value"]), dtype=torch.float32,
                                      device=p.device)
        return state

    def _row_step(self, p, ids, rows, state, group):
        state["step"] += 1
        ops.sparse_row_step("adagrad", p, ids, rows, (state["sum"],), lr=group["lr"], eps=group["eps"])


class SparseAdam(_SparseRowOptimizer):
    """Lazy Adam, the formula of torch.optim.SparseAdam: the moments and the parameter move only
    in the rows the gradient names; `step` counts every step() with a gradient, an empty one too."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        _need(lr >= 0.0, "learning rate: %r" % (lr,))
        _need(eps >= 0.0, "epsilon value: %r" % (eps,))
        _need(0.0 <= betas[0] < 1.0, "beta parameter at index 0: %r" % (betas[0],))
        _need(0.0 <= betas[1] < 1.0, "beta parameter at index 1: %r" % (betas[1],))
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))

    def _state_of(self, p, group):
        state = self.state[p]
        if "exp_avg" not in state:
            state["step"] = 0
            state["exp_avg"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            state["exp_avg_sq"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
        return state

    def _row_step(self, p, ids, rows, state, group):
        state["step"] += 1
        ops.sparse_row_step("adam", p, ids, rows, (state["exp_avg"], state["exp_avg_sq"]), lr=group["lr"],
                            eps=group["eps"], betas=group["betas"], step=int(state["step"]))


def _sgd(params, lr):
    return SparseSGD(params, lr, 0.0)


def _momentum(params, lr):
    return SparseSGD(params, lr, 0.9)


optimizers = {"sgd": _sgd, "momentum": _momentum, "adagrad": SparseAdagrad, "adam": SparseAdam}


def get(optimizer):
    """the optimiser factory of a name - sgd, momentum (0.9), adagrad, adam - as the reference's
    optimizers.get: called as factory(params, lr); None for a name it does not know"""
    return optimizers.get(optimizer)
