"""Adam trajectories through every optimizer-state event of a training run, in float64: the checker of `s3gaussian_amd.optim.Adam`
(tests/test_optim_trajectory_gpu.py); tests/test_optim_ref_cpu.py checks the checker.

TEST INFRASTRUCTURE ONLY: plain torch on the CPU, no torch.optim in the reference itself.

A SCRIPT (build_script) is a list of operations fixed before anything runs:
    ("lr", {group: lr})            the learning rates of the scheduled groups, written before every step
    ("step", {tensor: grad|None})  one optimizer step on prescribed float32 gradients (None: the tensor has no gradient)
    ("event", kind, payload)       surgery on the optimizer state between two steps (EVENTS)
Gradients, replacement values, masks and permutations come from one seeded generator and are never a function of the parameters,
so two float32 evaluations of a script cannot drift apart chaotically: what separates them is round-off alone.

run(script, subject) applies one script to one SUBJECT and returns {tensor: (p, m, v, step)} in float64:
    PlainAdam(float64)              the reference value: the formula of include/s3g_optim.h in double
    TorchSubject("torch32")         torch.optim.Adam in float32 on the CPU -- the reference implementation's own arithmetic.  Its
                                    distance from the float64 value is the yardstick the bar is made of
    TorchSubject("torch64")         torch.optim.Adam in float64 (holds PlainAdam to 1e-12, test_optim_ref_cpu.py)
    TorchSubject("s3g", device)     s3gaussian_amd.optim.Adam on the GPU, the code under test
    PlainAdam(float32, mutate=...)  a float32 restatement of csrc/adam.hip's operation order with ONE wrong reading (MUTANTS): what
                                    the bar must be able to see

THE BAR (compare): per tensor and each of p, m, v
    max |subject - f64|  <=  BAR_MARGIN x max |torch32 - f64|  +  one float32 ulp of the tensor's largest magnitude
and equal step counts.  Parameters start at 1e-3 randn -- comparable to the total displacement of a script -- so that the update
arithmetic is resolved: at unit scale the rounding of p itself (6e-8 p per step) hides a bias correction that is one step behind.

    python -m tests.optim_ref --report     runs every script on the GPU, writes profiles/adam_trajectory_errors.json"""
import copy
import json
import math
import os
import sys

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
BAR_MARGIN = 4.0
EVENTS = ("set_lr", "replace", "cat", "prune", "permute", "checkpoint_same", "checkpoint_fresh", "step_repr", "jump")
STEP_REPRS = ("fill", "cpu", "gpu", "float", "int", "cpu")   # in turn, one per step; "fill" changes the count in place by FILL_DELTA
FILL_DELTA = -3.0
JUMP_TO = 29990.0
MUTANTS = ("stale_step", "prev_lr", "skip_tail", "no_zero_at_replace", "no_permute_moments", "w2_f32", "gs_m_only")
GAUSSIANS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")     # share the leading dimension P; surgery hits them together
P0, P_CAT = 67, 13

# group -> lr (a number, or (init, final, max_steps) of the exponential schedule), betas, eps
GROUPS = {
    "xyz": dict(lr=(1.6e-4, 1.6e-6, 200), betas=(0.9, 0.999), eps=1e-15),
    "f_dc": dict(lr=2.5e-3, betas=(0.9, 0.999), eps=1e-15),
    "f_rest": dict(lr=1.25e-4, betas=(0.9, 0.999), eps=1e-15),
    "opacity": dict(lr=0.05, betas=(0.9, 0.999), eps=1e-15),          # the unit-scale group: the realistic case
    "scaling": dict(lr=5e-3, betas=(0.9, 0.999), eps=1e-15),
    "rotation": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-15),
    "deformation": dict(lr=(1.6e-4, 1.6e-6, 200), betas=(0.9, 0.999), eps=1e-15),
    "grid": dict(lr=(1.6e-3, 1.6e-5, 200), betas=(0.8, 0.99), eps=1e-15),     # other betas: a second launch per step
    "misc": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8),              # gradients of 1e-6: eps is 1 % of the denominator
}
# tensor -> group, shape (P: the Gaussian count), scale of the initial values, scale of the gradients
TENSORS = {
    "xyz": dict(group="xyz", shape=("P", 3), init=1e-3, grad=1e-6),
    "f_dc": dict(group="f_dc", shape=("P", 1, 3), init=1e-3, grad=1e-2),
    "f_rest": dict(group="f_rest", shape=("P", 15, 3), init=1e-3, grad=1e-4, zero_every=5),
    "opacity": dict(group="opacity", shape=("P", 1), init=1.0, grad=1e-1),
    "scaling": dict(group="scaling", shape=("P", 3), init=1e-3, grad=1e2),
    "rotation": dict(group="rotation", shape=("P", 4), init=1e-3, grad=1.0),
    "mlp_w": dict(group="deformation", shape=(64, 64), init=1e-3, grad=1e-3),
    "mlp_b": dict(group="deformation", shape=(33,), init=1e-3, grad=1e-5, no_grad=(0, 1, 2, 22, 23, 24, 25)),
    "planes": dict(group="grid", shape=(1, 32, 8, 16), init=1e-3, grad=1e1, channels_last=True),
    "grid_b": dict(group="grid", shape=(7,), init=1e-3, grad=1e-3),
    "misc": dict(group="misc", shape=(5, 1), init=1e-3, grad=1e-6),
}


def lr_at(lr, it):
    """Log-linear interpolation from lr_init to lr_final over max_steps (the shape of the reference's update_learning_rate)."""
    if not isinstance(lr, tuple):
        return lr
    init, final, max_steps = lr
    t = min(max(it / max_steps, 0.0), 1.0)
    return math.exp(math.log(init) * (1.0 - t) + math.log(final) * t)


# ---------------------------------------------------------------------------------------------------------------- scripts

def _shape(spec, P):
    return tuple(P if s == "P" else s for s in spec["shape"])


def _randn(gen, shape, scale, spec=None):
    t = torch.randn(shape, generator=gen, dtype=F32) * scale
    if spec is not None and spec.get("channels_last"):
        t = t.contiguous(memory_format=torch.channels_last)
    return t


def build_script(events, steps=40, seed=0, grad_scale=1.0, tensors=None, skip_tail_at=None):
    """events: {step index: event name or list of names}, applied BEFORE the step of that index."""
    tensors = TENSORS if tensors is None else tensors
    gen = torch.Generator().manual_seed(seed)
    P = P0
    groups = {}
    for name, spec in tensors.items():
        groups.setdefault(spec["group"], []).append(name)
    init = {name: _randn(gen, _shape(spec, P), spec["init"], spec) for name, spec in tensors.items()}
    gauss = [n for n in tensors if n in GAUSSIANS]
    ops, reprs = [], iter(STEP_REPRS)
    for it in range(steps):
        evs = events.get(it, ())
        for ev in ((evs,) if isinstance(evs, str) else evs):
            if ev == "replace":       # opacity reset: new values for one tensor, both moments zeroed, step count kept
                ops.append(("event", "replace", {"opacity": _randn(gen, _shape(tensors["opacity"], P), 0.1) - 2.0}))
            elif ev == "cat":         # densification: P_CAT new Gaussians with zero moments
                ops.append(("event", "cat", {n: _randn(gen, _shape(tensors[n], P_CAT), tensors[n]["init"]) for n in gauss}))
                P += P_CAT
            elif ev == "prune":
                mask = torch.rand(P, generator=gen) > 0.25
                ops.append(("event", "prune", (gauss, mask)))
                P = int(mask.sum())
            elif ev == "permute":
                ops.append(("event", "permute", (gauss, torch.randperm(P, generator=gen))))
            elif ev in ("checkpoint_same", "checkpoint_fresh"):
                ops.append(("event", "checkpoint", ev[len("checkpoint_"):]))
            elif ev == "step_repr":
                ops.append(("event", "step_repr", next(reprs)))
            elif ev == "jump":
                ops.append(("event", "jump", JUMP_TO))
            else:
                raise KeyError(ev)
        ops.append(("lr", {g: lr_at(GROUPS[g]["lr"], it) for g in groups if isinstance(GROUPS[g]["lr"], tuple)}))
        grads = {}
        for name, spec in tensors.items():
            if it in spec.get("no_grad", ()):
                grads[name] = None
                continue
            g = _randn(gen, _shape(spec, P), spec["grad"], spec)
            if spec.get("zero_every"):
                g.view(-1)[::spec["zero_every"]] = 0.0
            grads[name] = g
        ops.append(("step", grads))
    return dict(tensors=tensors, groups=groups, init=init, ops=ops, grad_scale=grad_scale, skip_tail_at=skip_tail_at)


def event_script(event):
    """One event in the middle of 40 steps, several steps before it and after it."""
    if event == "set_lr":            # nothing but the schedule
        return build_script({}, seed=11, grad_scale=0.125)
    if event == "step_repr":
        return build_script({16 + k: "step_repr" for k in range(len(STEP_REPRS))}, seed=12)
    if event == "jump":              # a run resumed late: ten steps at 29 990
        return build_script({30: "jump"}, seed=13)
    return build_script({20: event}, seed=20 + EVENTS.index(event))


def full_script():
    ev = {8: "replace", 13: "cat", 18: "prune", 23: "permute", 28: "checkpoint_same", 32: "checkpoint_fresh", 50: "jump"}
    ev.update({36 + k: "step_repr" for k in range(len(STEP_REPRS))})
    return build_script(ev, steps=60, seed=1, grad_scale=0.125, skip_tail_at=45)


SHAPE_NUMELS = (0, 1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025)
BIG_NUMEL = 2_097_152 + 3 * 1024 + 3      # 2048 workgroups x 256 lanes x 4 elements, and a short third pass of the grid-stride loop


def shapes_script():
    """Every tail length and the sizes around one workgroup, three steps, one group (one launch): the big tensor sets the grid, the
    small tensors' rows of workgroups have nothing to do."""
    tensors = {f"n{n}": dict(group="f_dc", shape=(n,), init=1e-3, grad=1e-2) for n in SHAPE_NUMELS + (BIG_NUMEL,)}
    return build_script({}, steps=3, seed=2, tensors=tensors)


ALIGN_KINDS = ("param", "grad", "exp_avg", "exp_avg_sq")
ALIGN_N = 1028       # + r: two workgroups per row; everything goes through the scalar loop when one pointer is off


def align_script():
    """-> (script, {tensor: {kind: element offset}}): each of the four arrays in turn the only one off a 16-byte boundary (offset 1, 2,
    3), with numel % 4 in {0, 1, 2, 3}; all four off by the same offset; and all four on a boundary at offset 4."""
    tensors, offsets = {}, {}
    for r in range(4):
        for off in (1, 2, 3):
            for kind in ALIGN_KINDS:
                name = f"{kind}_o{off}_r{r}"
                tensors[name] = dict(group="f_dc" if r % 2 else "rotation", shape=(ALIGN_N + r,), init=1e-3, grad=1e-2)
                offsets[name] = {k: (off if k == kind else 0) for k in ALIGN_KINDS}
            name = f"all_o{off}_r{r}"
            tensors[name] = dict(group="rotation", shape=(ALIGN_N + r,), init=1e-3, grad=1e-2)
            offsets[name] = {k: off for k in ALIGN_KINDS}
        name = f"all_o4_r{r}"
        tensors[name] = dict(group="f_dc", shape=(ALIGN_N + r,), init=1e-3, grad=1e-2)
        offsets[name] = {k: 4 for k in ALIGN_KINDS}
    return build_script({}, steps=3, seed=3, tensors=tensors), offsets


def repoint_script(case):
    """`p.data` of the SAME Parameter moved to another size / shape at the same address after three steps, three more steps after it.
    Payload: (tensor, new shape, values of the elements that become live | None)."""
    old, new = {"shrink": ((12,), (8,)), "grow": ((8,), (12,)), "restride": ((6, 2), (4, 3))}[case]
    gen = torch.Generator().manual_seed(40 + len(case))
    spec = dict(group="rotation", init=1e-3, grad=1e-2)
    tensors = {"t": dict(spec, shape=old), "other": dict(spec, shape=(9,))}
    s = build_script({}, steps=3, seed=4, tensors=tensors)
    grown = int(np.prod(new)) - int(np.prod(old))
    ext = torch.randn(grown, generator=gen) * 1e-3 if grown > 0 else None
    s["ops"].append(("event", "repoint", ("t", new, ext)))
    for _ in range(3):
        s["ops"].append(("step", {"t": _randn(gen, new, 1e-2), "other": _randn(gen, (9,), 1e-2)}))
    return s


# ------------------------------------------------------------------------------------------------------ the plain reference

class PlainAdam:
    """Adam over named tensors in groups with the fields of torch.optim.Adam (lr, betas, eps; per tensor step, exp_avg, exp_avg_sq).
    dtype float64: the formula of include/s3g_optim.h, the reference value.  dtype float32: csrc/adam.hip restated -- its operation
    order, its scalars rounded where the kernel rounds them; `fma` contracts where a compiler may; `mutate` (MUTANTS) makes one wrong
    reading.  A tensor whose gradient is None is left alone and its step count does not advance."""

    def __init__(self, script, dtype=F64, mutate=None, fma=False):
        assert mutate is None or mutate in MUTANTS
        self.dtype, self.mutate, self.fma = dtype, mutate, fma
        self.group_of = {n: spec["group"] for n, spec in script["tensors"].items()}
        self.groups = {g: dict(GROUPS[g], lr=lr_at(GROUPS[g]["lr"], 0)) for g in script["groups"]}
        self.p = {n: t.to(dtype).contiguous().clone() for n, t in script["init"].items()}
        self.m, self.v, self.steps = {}, {}, {}
        self.grad_scale = script["grad_scale"]
        self.skip_tail_at, self.calls = script["skip_tail_at"], 0
        self.lag, self.lr_used = 0.0, {g: self.groups[g]["lr"] for g in self.groups}

    def set_lr(self, lrs):
        for g, lr in lrs.items():
            self.lr_used[g] = self.groups[g]["lr"] if self.mutate == "prev_lr" else lr
            self.groups[g]["lr"] = lr

    def step(self, grads):
        for n, g in grads.items():
            if g is None:
                continue
            if n not in self.m:
                self.m[n], self.v[n], self.steps[n] = torch.zeros_like(self.p[n]), torch.zeros_like(self.p[n]), 0.0
            self.steps[n] += 1.0
            grp = self.groups[self.group_of[n]]
            lr = self.lr_used[self.group_of[n]] if self.mutate == "prev_lr" else grp["lr"]
            (self._update_f64 if self.dtype is F64 else self._update_f32)(n, g.contiguous(), lr, grp["betas"], grp["eps"],
                                                                           self.steps[n] - self.lag)
        self.calls += 1

    def _update_f64(self, n, g, lr, betas, eps, t):
        b1, b2 = betas
        p, m, v = self.p[n], self.m[n], self.v[n]
        g = g.to(F64) * self.grad_scale
        m += (g - m) * (1.0 - b1)
        v.mul_(b2).add_((1.0 - b2) * g * g)
        p -= (lr / (1.0 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)

    def _update_f32(self, n, g, lr, betas, eps, t):
        b1, b2 = betas
        f = lambda x: torch.tensor(x, dtype=F32)
        w1, w2, b2f = f(1.0 - b1), f(1.0 - b2), f(b2)          # 1 - beta in double, rounded once (AdamArgs)
        if self.mutate == "w2_f32":
            w2 = f(1.0) - f(b2)
        step_size, isb, eps, gs = f(lr / (1.0 - b1 ** t)), f(1.0 / math.sqrt(1.0 - b2 ** t)), f(eps), f(self.grad_scale)
        p, m, v = self.p[n].view(-1), self.m[n].view(-1), self.v[n].view(-1)
        live = p.numel()
        if self.mutate == "skip_tail" and self.calls == self.skip_tail_at:
            live -= live % 4
        p, m, v, gu = p[:live], m[:live], v[:live], g.view(-1)[:live]
        g = gu * gs
        gv = gu if self.mutate == "gs_m_only" else g
        if self.fma:          # a * b + c with one rounding: the product of two float32 is exact in double
            fma = lambda a, b, c: (a.double() * b.double() + c.double()).float()
            m.copy_(fma(g - m, w1, m))
            v.copy_(fma(w2 * gv, gv, b2f * v))
            denom = fma(v.sqrt(), isb, eps)
            p.copy_(fma(-step_size, m / denom, p))
        else:
            m.copy_(m + (g - m) * w1)
            v.copy_(b2f * v + w2 * gv * gv)
            denom = v.sqrt() * isb + eps
            p.copy_(p - step_size * (m / denom))

    def event(self, kind, payload):
        if self.mutate == "stale_step":
            self.lag = 1.0            # from here on the bias corrections are one step behind; the reported count is right
        has = lambda n: n in self.m
        if kind == "replace":
            for n, val in payload.items():
                self.p[n] = val.to(self.dtype).clone()
                if has(n) and self.mutate != "no_zero_at_replace":
                    self.m[n], self.v[n] = torch.zeros_like(self.p[n]), torch.zeros_like(self.p[n])
        elif kind == "cat":
            for n, ext in payload.items():
                self.p[n] = torch.cat([self.p[n], ext.to(self.dtype)])
                if has(n):
                    z = torch.zeros_like(ext, dtype=self.dtype)
                    self.m[n], self.v[n] = torch.cat([self.m[n], z]), torch.cat([self.v[n], z])
        elif kind in ("prune", "permute"):
            names, idx = payload
            for n in names:
                self.p[n] = self.p[n][idx].clone()
                if has(n) and not (kind == "permute" and self.mutate == "no_permute_moments"):
                    self.m[n], self.v[n] = self.m[n][idx].clone(), self.v[n][idx].clone()
        elif kind == "checkpoint":
            pass                      # saving and loading changes nothing
        elif kind == "step_repr":
            if payload == "fill":
                self.steps = {n: s + FILL_DELTA for n, s in self.steps.items()}
        elif kind == "jump":
            self.steps = {n: float(payload) for n in self.steps}
        elif kind == "repoint":
            n, shape, ext = payload
            numel = int(np.prod(shape))
            for d, fill in ((self.p, ext), (self.m, None), (self.v, None)):
                if n in d:
                    flat = d[n].reshape(-1)
                    if numel > flat.numel():
                        tail = fill.to(self.dtype) if fill is not None else torch.zeros(numel - flat.numel(), dtype=self.dtype)
                        flat = torch.cat([flat, tail])
                    d[n] = flat[:numel].reshape(shape).clone()
        else:
            raise KeyError(kind)

    def result(self):
        return {n: (p.to(F64), self.m[n].to(F64) if n in self.m else None, self.v[n].to(F64) if n in self.v else None,
                    self.steps.get(n, 0.0)) for n, p in self.p.items()}


# ------------------------------------------------------------------------------------ subjects with torch.optim's state layout

class TorchSubject:
    """A script applied to an optimizer with torch.optim.Adam's state layout: torch.optim.Adam itself on the CPU ("torch32",
    "torch64") or s3gaussian_amd.optim.Adam on `device` ("s3g").  The surgery is what a training loop does to `opt.state` and
    `opt.param_groups`, written from the description of each event.

    place(name, kind, numel) -> a flat float32 device tensor of numel elements (a view into memory the caller owns), kind in
    ALIGN_KINDS: parameters, gradients and moments of the s3g subject are then put there instead of into fresh allocations."""

    def __init__(self, script, kind, device="cpu", place=None):
        self.kind, self.device, self.place = kind, torch.device(device), place
        self.dtype = F64 if kind == "torch64" else F32
        self.names = list(script["tensors"])
        self.grad_scale = script["grad_scale"]
        self.params = {n: torch.nn.Parameter(self._put(n, "param", t.to(self.dtype))) for n, t in script["init"].items()}
        groups = [dict(params=[self.params[n] for n in names], name=g, lr=lr_at(GROUPS[g]["lr"], 0), betas=GROUPS[g]["betas"],
                       eps=GROUPS[g]["eps"]) for g, names in script["groups"].items()]
        self.opt = self._optimizer(groups)
        if place is not None:         # the moments live where the caller wants them: state as after torch's lazy initialisation
            for n, p in self.params.items():
                self.opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": self._put(n, "exp_avg", torch.zeros_like(p)),
                                     "exp_avg_sq": self._put(n, "exp_avg_sq", torch.zeros_like(p))}

    def _optimizer(self, groups):
        if self.kind == "s3g":
            from s3gaussian_amd.optim import Adam
            opt = Adam(groups, lr=0.0)
            opt.grad_scale = self.grad_scale
            return opt
        return torch.optim.Adam(groups, lr=0.0, foreach=False)

    def _put(self, name, kind, t):
        t = t.detach()
        if self.place is None:
            return t.to(self.device, copy=True)       # never the script's own tensor: the optimizer writes in place
        dst = self.place(name, kind, t.numel())
        dst.copy_(t.reshape(-1))
        return dst.view(t.shape)

    def _name(self, p):
        return next(n for n, q in self.params.items() if q is p)

    def set_lr(self, lrs):
        for group in self.opt.param_groups:
            if group["name"] in lrs:
                group["lr"] = lrs[group["name"]]

    def step(self, grads):
        for n, g in grads.items():
            if g is None:
                self.params[n].grad = None
            elif self.kind == "s3g":
                self.params[n].grad = self._put(n, "grad", g)
            else:      # torch.optim.Adam has no grad_scale: scale in float32, as the kernel does (exact for a power of two)
                self.params[n].grad = (g * torch.tensor(self.grad_scale, dtype=F32)).to(self.dtype)
        self.opt.step()

    def _swap(self, name, new):
        """A new Parameter takes the place of the old one in its group and inherits its state dict OBJECT."""
        old, new = self.params[name], torch.nn.Parameter(new.clone())     # (a payload must not become a parameter's storage)
        for group in self.opt.param_groups:
            group["params"] = [new if q is old else q for q in group["params"]]
        st = self.opt.state.pop(old, None)
        if st is not None:
            self.opt.state[new] = st
        self.params[name] = new
        return st

    def event(self, kind, payload):
        opt, dev = self.opt, self.device
        if kind == "replace":
            for n, val in payload.items():
                st = self._swap(n, val.to(dev, self.dtype))
                if st is not None:
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(self.params[n]), torch.zeros_like(self.params[n])
        elif kind == "cat":
            for n, ext in payload.items():
                ext = ext.to(dev, self.dtype)
                st = self._swap(n, torch.cat([self.params[n].detach(), ext]))
                if st is not None:
                    st["exp_avg"] = torch.cat([st["exp_avg"], torch.zeros_like(ext)])
                    st["exp_avg_sq"] = torch.cat([st["exp_avg_sq"], torch.zeros_like(ext)])
        elif kind == "prune":
            names, mask = payload
            mask = mask.to(dev)
            for n in names:
                st = self._swap(n, self.params[n].detach()[mask])
                if st is not None:
                    st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][mask], st["exp_avg_sq"][mask]
        elif kind == "permute":       # the Parameter keeps its identity
            names, perm = payload
            perm = perm.to(dev)
            for n in names:
                p = self.params[n]
                p.data = p.data[perm].contiguous()
                st = opt.state.get(p)
                if st is not None:
                    st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][perm].contiguous(), st["exp_avg_sq"][perm].contiguous()
        elif kind == "checkpoint":
            sd = copy.deepcopy(opt.state_dict())
            if payload == "same":
                opt.load_state_dict(sd)
            else:                     # a fresh optimizer over fresh copies of the parameters, in the saved order
                fresh = {n: torch.nn.Parameter(p.detach().clone()) for n, p in self.params.items()}
                groups = [dict(params=[fresh[self._name(q)] for q in g["params"]], name=g["name"], lr=0.0, betas=(0.5, 0.5), eps=1.0)
                          for g in opt.param_groups]
                self.params, self.opt = fresh, self._optimizer(groups)
                self.opt.load_state_dict(sd)
        elif kind == "step_repr":
            for st in opt.state.values():
                val = float(st["step"])
                if payload == "fill":
                    st["step"].fill_(val + FILL_DELTA)
                elif self.kind == "s3g":      # torch.optim.Adam itself needs a tensor here; the value is the same
                    st["step"] = {"cpu": lambda: torch.tensor(val), "gpu": lambda: torch.tensor(val, device=dev),
                                  "float": lambda: val, "int": lambda: int(val)}[payload]()
        elif kind == "jump":
            for st in opt.state.values():
                st["step"] = torch.tensor(float(payload))
        elif kind == "repoint":
            n, shape, ext = payload
            numel, p = int(np.prod(shape)), self.params[n]
            if self.place is None:    # the CPU subjects: a new Parameter, moments cut or extended by zeros
                grow = lambda t, tail: torch.cat([t.reshape(-1), tail.to(t)])[:numel].reshape(shape).clone()
                z = torch.zeros(max(numel - p.numel(), 0))
                st = self._swap(n, grow(p.detach(), ext if ext is not None else z))
                st["exp_avg"], st["exp_avg_sq"] = grow(st["exp_avg"], z), grow(st["exp_avg_sq"], z)
            else:                     # the subject under test: the SAME Parameter, p.data re-pointed at the same address
                st, old = opt.state[p], p.numel()
                for k, tail in (("param", ext), ("exp_avg", None), ("exp_avg_sq", None)):
                    buf = self.place(n, k, max(numel, old))
                    if numel > old:
                        buf[old:] = tail.to(dev) if tail is not None else 0.0
                    view = self.place(n, k, numel).view(shape)
                    if k == "param":
                        assert view.data_ptr() == p.data_ptr()
                        p.grad = None
                        p.data = view
                    else:
                        st[k] = view
        else:
            raise KeyError(kind)

    def result(self):
        out = {}
        for n, p in self.params.items():
            st = self.opt.state.get(p) or {}
            get = lambda t: None if t is None else t.detach().to("cpu", F64)
            if self.place is not None:        # what is in the caller's memory, not what the state dict points to
                q = lambda k: self.place(n, k, p.numel()).view(p.shape)
                out[n] = (get(q("param")), get(q("exp_avg")), get(q("exp_avg_sq")), float(st.get("step", 0.0)))
            else:
                out[n] = (get(p), get(st.get("exp_avg")), get(st.get("exp_avg_sq")), float(st.get("step", 0.0)))
        return out


def run(script, subject):
    for op in script["ops"]:
        if op[0] == "lr":
            subject.set_lr(op[1])
        elif op[0] == "step":
            subject.step(op[1])
        else:
            subject.event(op[1], op[2])
    return subject.result()


_yardsticks = {}


def yardsticks(key, script):
    """(float64 reference, torch.optim.Adam float32) results of a script, computed once per process and left unchanged."""
    if key not in _yardsticks:
        _yardsticks[key] = (run(script, PlainAdam(script, F64)), run(script, TorchSubject(script, "torch32")))
    return _yardsticks[key]


# ---------------------------------------------------------------------------------------------------------------- the bar

def _maxabs(t):
    return float(t.abs().max()) if t is not None and t.numel() else 0.0


def compare(sub, f64, cpu32):
    """-> rows {tensor, quantity, err_cpu32, err, ratio, bar, ok}, one per tensor and each of p, m, v, step."""
    rows = []
    assert set(sub) == set(f64) == set(cpu32)
    for n in f64:
        for k, q in enumerate(("p", "m", "v")):
            want, a, b = f64[n][k], cpu32[n][k], sub[n][k]
            if want is None or a is None or b is None:
                rows.append(dict(tensor=n, quantity=q, err_cpu32=None, err=None, ratio=None, bar=None,
                                 ok=want is None and a is None and b is None))
                continue
            if not (want.shape == a.shape == b.shape):
                rows.append(dict(tensor=n, quantity=q, err_cpu32=None, err=None, ratio=None, bar=None, ok=False,
                                 shapes=[list(want.shape), list(a.shape), list(b.shape)]))
                continue
            e_cpu, e_sub = _maxabs(a - want), _maxabs(b - want)
            if not math.isfinite(e_sub):
                e_sub = math.inf
            bar = BAR_MARGIN * e_cpu + float(np.spacing(np.float32(_maxabs(want))))
            rows.append(dict(tensor=n, quantity=q, err_cpu32=e_cpu, err=e_sub, ratio=(e_sub / e_cpu if e_cpu > 0 else None), bar=bar,
                             ok=e_sub <= bar))
        steps = (f64[n][3], cpu32[n][3], sub[n][3])
        rows.append(dict(tensor=n, quantity="step", err_cpu32=None, err=None, ratio=None, bar=None, steps=list(steps),
                         ok=steps[0] == steps[1] == steps[2]))
    return rows


def worst_over_bar(rows):
    """Largest err / bar over the rows (inf if a step count or a shape differs)."""
    worst = 0.0
    for r in rows:
        if r["bar"] is None:
            worst = worst if r["ok"] else math.inf
        else:
            worst = max(worst, r["err"] / r["bar"] if r["bar"] > 0 else (0.0 if r["err"] == 0 else math.inf))
    return worst


def largest_ratio(rows):
    return max((r["ratio"] for r in rows if r["ratio"] is not None), default=0.0)


def table(rows, only_failed=False):
    lines = [f"{'tensor':<22}{'':>5}{'cpu32-f64':>12}{'subject-f64':>13}{'ratio':>11}{'bar':>12}"]
    for r in rows:
        if only_failed and r["ok"]:
            continue
        if r["bar"] is None:
            lines.append(f"{r['tensor']:<22}{r['quantity']:>5}  {r.get('steps', r.get('shapes', ''))}  {'ok' if r['ok'] else 'DIFFERENT'}")
        else:
            ratio = "-" if r["ratio"] is None else f"{r['ratio']:.3g}"
            lines.append(f"{r['tensor']:<22}{r['quantity']:>5}{r['err_cpu32']:>12.3e}{r['err']:>13.3e}{ratio:>11}{r['bar']:>12.3e}"
                         f"{'' if r['ok'] else '  OVER'}")
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------- the subject under test

class OwnedBuffers:
    """Flat float32 device buffers the caller owns, one per (tensor, kind), each `pad` elements longer than the tensor at both ends
    and filled with a pattern: place() hands out the view at the tensor's element offset; untouched() says whether everything
    outside the views still holds the pattern, bit for bit."""

    def __init__(self, device, capacity, offsets=None, pad=8):
        self.device, self.capacity, self.offsets, self.pad = device, capacity, offsets or {}, pad
        self.bufs, self.live = {}, {}

    def _pattern(self, n):
        return 0.5 + torch.arange(n, dtype=F32, device=self.device) * 2.0 ** -10

    def place(self, name, kind, numel):
        key = (name, kind)
        if key not in self.bufs:
            self.bufs[key] = self._pattern(self.capacity[name] + 2 * self.pad)
        off = self.pad + self.offsets.get(name, {}).get(kind, 0) - (self.pad % 4)     # pad 8: offset 0 is 16-byte aligned
        prev = self.live.get(key, (off, 0))[1]
        if prev > numel:              # the view shrinks: what it leaves behind holds the pattern again
            self.bufs[key][off + numel:off + prev] = self._pattern(off + prev)[off + numel:]
        self.live[key] = (off, numel)
        return self.bufs[key][off:off + numel]

    def untouched(self):
        bad = []
        for key, buf in self.bufs.items():
            off, numel = self.live[key]
            want = self._pattern(buf.numel())
            same = buf.view(torch.int32) == want.view(torch.int32)
            same[off:off + numel] = True
            if not bool(same.all()):
                bad.append((key, torch.nonzero(~same).flatten().tolist()))
        return bad


def gpu_rows(name, device):
    """One named script on the subject under test -> (rows, OwnedBuffers | None)."""
    bufs = None
    if name == "shapes":
        script = shapes_script()
    elif name == "align":
        script, offsets = align_script()
        bufs = OwnedBuffers(device, {n: _shape(s, 0)[0] for n, s in script["tensors"].items()}, offsets)
    elif name.startswith("repoint_"):
        script = repoint_script(name[len("repoint_"):])
        bufs = OwnedBuffers(device, {"t": 12, "other": 9})
    elif name == "all":
        script = full_script()
    else:
        script = event_script(name)
    f64, cpu32 = yardsticks(name, script)
    sub = run(script, TorchSubject(script, "s3g", device, place=bufs.place if bufs is not None else None))
    return compare(sub, f64, cpu32), bufs


GPU_SCRIPTS = EVENTS + ("all", "shapes", "align", "repoint_shrink", "repoint_grow", "repoint_restride")


def report(path):
    assert torch.cuda.is_available(), "--report runs the scripts on the GPU"
    dev = torch.device("cuda:0")
    sig = lambda x: None if x is None else float(f"{x:.4g}")
    out = {"bar": f"err_gpu <= {BAR_MARGIN:g} * err_cpu32 + ulp32(max |f64|); errors are max |x - f64| per tensor and quantity",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "scripts": {}}
    for name in GPU_SCRIPTS:
        rows, _ = gpu_rows(name, dev)
        rows = [r for r in rows if r["bar"] is not None]
        out["scripts"][name] = {"largest_ratio": sig(largest_ratio(rows)), "worst_err_over_bar": sig(worst_over_bar(rows)),
                                "rows": [dict(tensor=r["tensor"], quantity=r["quantity"], err_cpu32=sig(r["err_cpu32"]),
                                              err_gpu=sig(r["err"]), ratio=sig(r["ratio"])) for r in rows]}
    out["largest_ratio"] = max(s["largest_ratio"] for s in out["scripts"].values())
    out["worst_err_over_bar"] = max(s["worst_err_over_bar"] for s in out["scripts"].values())
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"largest ratio {out['largest_ratio']}, worst err / bar {out['worst_err_over_bar']} -> {path}")


if __name__ == "__main__":
    if "--report" in sys.argv[1:]:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        report(os.path.join(root, "profiles", "adam_trajectory_errors.json"))
    else:
        sys.exit(__doc__)
