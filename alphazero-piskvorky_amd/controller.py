"""controller.py seam (controller.py:33-207): make_policy_value_fn evaluates on the GPU engine;
NeuralNetworkController keeps the reference's training surface (torch AdamW, soft-target CE + MSE)."""
import numpy as np
import torch
import torch.nn.functional as F

from . import constants as _c
from ._capi import Engine
from .games import Gomoku


class PolicyValueFn:
    """Callable state -> (P float32[n,n], float v) (controller.py:39-53).  Carries the controller so that
    MCTS / SelfPlayManager can hand its weights to the engine instead of calling back into Python per leaf."""

    def __init__(self, controller):
        self.controller = controller
        self._engine = None
        self._version = None

    def _eng(self, n):
        ver = weights_version(self.controller.net)
        if self._engine is None or self._engine.n != n:
            self._engine = Engine(n, min(_c.WIN_LENGTH, n), 1, 1, device=device_index(self.controller.device),
                                  model=model_kind(self.controller.net))
            self._version = None
        if ver != self._version:
            self._engine.load_weights(self.controller.net.state_dict(), 0)
            self._version = ver
        return self._engine

    def __call__(self, state):
        if not isinstance(state, Gomoku):
            raise TypeError("policy_value_fn expects a Gomoku state")
        n = state.board_size
        _, P, v = self._eng(n).net_eval(state.cells[None], [state.player_code()], [state.last_index()])
        return P[0].reshape(n, n), float(v[0])


def make_policy_value_fn(controller):
    return PolicyValueFn(controller)


class BatchPolicyValueFn:
    """The evaluator seam for ANY net on the engine's GPU, every game at once (az_set_external_evaluator):
        fn(planes: cuda float32 tensor [count, 4, n, n], net: int) -> (policy [count, n*n] or [count, n, n], value [count] or [count, 1])
    planes are Gomoku.encode of the positions that wait for an evaluation (games.py:86-129; plane 0 the side to move), a view
    into this object's buffer that is valid during the call only; policy is used as priors exactly as given (mcts.py:63) and
    value is for the side to move.  net is 0, in the arena 0 = candidate / 1 = baseline.  The object owns the three device
    buffers the engine reads and writes, sizes them from Engine.ext_capacity(), copies fn's results in and synchronises the
    current torch stream before it returns to the engine.  MCTS, SelfPlayManager(evaluator=...) and
    ModelEvaluator(evaluators=...) take one."""

    def __init__(self, fn, device=None):
        if not callable(fn):
            raise TypeError("fn must be callable: fn(planes [count, 4, n, n], net) -> (policy, value)")
        self.fn = fn
        self.device = torch.device("cuda", device_index(device))
        self._buffers = {}            # per attached engine: (planes, policy, value)

    def __call__(self, planes, net=0):
        return self.fn(planes, net)

    def attach(self, engine):
        """Make this object the evaluator of `engine`; call again after set_virtual_loss (the capacity follows it)."""
        n, nn, cap = engine.n, engine.nn, engine.ext_capacity()
        if device_index(self.device) != engine.device:
            raise ValueError(f"the evaluator lives on {self.device}, the engine on cuda:{engine.device}")
        planes = torch.zeros((cap, 4, n, n), dtype=torch.float32, device=self.device)
        policy = torch.zeros((cap, nn), dtype=torch.float32, device=self.device)
        value = torch.zeros(cap, dtype=torch.float32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()

        def serve(net, count):
            with torch.cuda.device(self.device):
                P, v = self.fn(planes[:count], net)
                policy[:count].copy_(torch.as_tensor(P, dtype=torch.float32).reshape(count, nn))
                value[:count].copy_(torch.as_tensor(v, dtype=torch.float32).reshape(count))
                torch.cuda.current_stream(self.device).synchronize()      # complete in device memory before the engine reads

        engine.set_external_evaluator(planes.data_ptr(), policy.data_ptr(), value.data_ptr(), cap, serve)
        self._buffers[id(engine)] = (planes, policy, value)
        return engine

    def detach(self, engine):
        engine.clear_external_evaluator()
        self._buffers.pop(id(engine), None)


def make_batch_policy_value_fn(module_or_pair, device=None):
    """BatchPolicyValueFn for any nn.Module with the reference's forward contract, planes [B, 4, n, n] -> (logits [B, n*n],
    value [B, 1] or [B]) (net.py:55-72): evaluated under torch.no_grad() with softmax over the n*n logits, as
    controller.py:44-49 does for one state.  A pair is (candidate, baseline) for the arena.
    The number of positions that wait for the net changes from request to request, and a convolution library that tunes or
    compiles per input shape would do so for every new count: the module is therefore shown batches of a few sizes only --
    the request copied into a scratch tensor of the next power of two rows (at least 16; rows behind the request hold
    zeros or older positions, their results are dropped)."""
    mods = tuple(module_or_pair) if isinstance(module_or_pair, (tuple, list)) else (module_or_pair,)
    if len(mods) not in (1, 2) or not all(isinstance(m, torch.nn.Module) for m in mods):
        raise TypeError("make_batch_policy_value_fn takes an nn.Module or a (candidate, baseline) pair of them")
    if device is None:
        device = next(mods[0].parameters()).device
    scratch = {}

    def fn(planes, net):
        count = planes.shape[0]
        rows = 16
        while rows < count:
            rows *= 2
        key = (rows, tuple(planes.shape[1:]), planes.device)
        if key not in scratch:
            scratch[key] = torch.zeros((rows,) + tuple(planes.shape[1:]), dtype=planes.dtype, device=planes.device)
        batch = scratch[key]
        batch[:count].copy_(planes)
        with torch.no_grad():
            logits, value = mods[net if len(mods) == 2 else 0](batch)
            return torch.softmax(logits[:count], dim=1), value[:count]

    return BatchPolicyValueFn(fn, device)


def merge_batch_evaluators(evaluators):
    """One BatchPolicyValueFn from a (candidate, baseline) pair of them: request `net` goes to evaluators[net]."""
    if isinstance(evaluators, BatchPolicyValueFn):
        return evaluators
    pair = tuple(evaluators)
    if len(pair) != 2 or not all(isinstance(x, BatchPolicyValueFn) for x in pair):
        raise TypeError("evaluators must be a BatchPolicyValueFn or a (candidate, baseline) pair of them")
    return BatchPolicyValueFn(lambda planes, net: pair[net].fn(planes, net), pair[0].device)


def model_kind(net):
    from .net import GomokuResNet
    return "resnet" if isinstance(net, GomokuResNet) else "plain"


def device_index(device):
    d = torch.device(device) if device is not None else torch.device("cuda")
    return d.index if d.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)


def weights_version(net):
    return tuple((p.data_ptr(), p._version) for p in net.state_dict().values())


class AlphaZeroDataset(torch.utils.data.Dataset):
    def __init__(self, examples):
        self.examples = examples

    def __len__(self):
        return len(self.examples)

    def __getitem__(self, i):
        s, p, z = self.examples[i]
        return s.float(), p, (z.float() if torch.is_tensor(z) else torch.tensor(z, dtype=torch.float32))


class NeuralNetworkController:
    def __init__(self, net, device=None, lr=None, batch_size=None):
        self.net = net
        self.device = device if device is not None else "cuda"
        self.batch_size = batch_size or _c.BATCH_SIZE
        self.net.to(self.device)
        self.optimizer = torch.optim.AdamW(self.net.parameters(), lr=lr or _c.LEARNING_RATE, weight_decay=1e-4)
        self.training_history = []

    def train_step(self, states, pis, zs):
        """One optimizer step (controller.py:100-131): loss = CE(soft pi) + MSE(z)."""
        self.net.train()
        states, pis, zs = states.to(self.device), pis.to(self.device), zs.to(self.device)
        logits, value = self.net(states)
        policy_loss = -(pis.flatten(1) * F.log_softmax(logits, dim=1)).sum(dim=1).mean()
        value_loss = F.mse_loss(value.squeeze(-1), zs)
        loss = policy_loss + value_loss
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        return {"loss": loss.item(), "policy_loss": policy_loss.item(), "value_loss": value_loss.item()}

    def train(self, examples, epochs=1):
        n = self.net.board_size
        examples = list(examples)                       # sample_batch may hand over the deque itself
        for s, _, _ in examples[:1]:
            if tuple(s.shape) != (4, n, n):
                raise ValueError(f"example state has shape {tuple(s.shape)}, expected {(4, n, n)}")   # controller.py:136-138
        loader = torch.utils.data.DataLoader(AlphaZeroDataset(examples), batch_size=self.batch_size, shuffle=True)
        for _ in range(epochs):
            sums, batches = {}, 0
            for states, pis, zs in loader:
                out = self.train_step(states, torch.as_tensor(pis), zs)
                for k, v in out.items():
                    sums[k] = sums.get(k, 0.0) + v
                batches += 1
            self.training_history.append({k: v / max(batches, 1) for k, v in sums.items()})
        self.net.eval()
        return self.training_history[-1] if self.training_history else {}

    def train_tensors(self, states, pis, zs, epochs=1):
        """train() for a batch that is already on the device as tensors (device_replay.DeviceReplayBuffer.sample_batch):
        the same epochs of shuffled mini-batches of `batch_size` (controller.py:140-194), no Dataset / DataLoader hop."""
        n = self.net.board_size
        if tuple(states.shape[1:]) != (4, n, n):
            raise ValueError(f"example state has shape {tuple(states.shape[1:])}, expected {(4, n, n)}")
        total = states.shape[0]
        for _ in range(epochs):
            perm = torch.randperm(total, device=states.device)
            sums, batches = {}, 0
            for lo in range(0, total, self.batch_size):
                idx = perm[lo:lo + self.batch_size]
                out = self.train_step(states[idx], pis[idx], zs[idx])
                for k, v in out.items():
                    sums[k] = sums.get(k, 0.0) + v
                batches += 1
            self.training_history.append({k: v / max(batches, 1) for k, v in sums.items()})
        self.net.eval()
        return self.training_history[-1] if self.training_history else {}

    def save(self, path):
        torch.save(self.net.state_dict(), path)

    def load(self, path):
        self.net.load_state_dict(torch.load(path, map_location=self.device, weights_only=True))
