"""The library's own optimizer: Adam as the reference trains with it (coco_scripts/train.py:77-78,113: Adam(model.parameters(), lr=opt.lr)
plus StepLR), as ONE library call per step.

    optim = vsrcap.optim.Adam(model, lr=5e-4)            # instead of torch.optim.Adam(model.parameters(), lr=5e-4)
    scheduler = StepLR(optim, step_size=3, gamma=0.8)    # unchanged: param_groups[0]['lr'] is read at every step

vsr_adam_step (include/vsrcap.h, csrc/optim_kernels.h) updates all 28 tensors in one launch and, in the same pass, leaves what the
engine derives from the weights - the fp16-pair images' bounds, the bf16 copies - so the training forward that follows issues no refresh
(models/controllable_captioning.py, "the weights' GENERATION", has the rules and what voids the shortcut).  torch.optim.Adam keeps
working exactly as before; this class is for callers who opt in.

The state per parameter is torch's - 'step' (a float32 scalar tensor, kept on the CPU while this class steps), 'exp_avg', 'exp_avg_sq' - so
state_dict() / load_state_dict() interchange with torch.optim.Adam checkpoints in both directions.  step(closure), the step hooks and
zero_grad are torch.optim.Optimizer's.  There is no eager fallback: CPU parameters raise."""
import torch

from . import _lib


class Adam(torch.optim.Optimizer):
    # the step leaves the model's derived weight state current: nobody has to void it afterwards (the process-wide step count of
    # models/controllable_captioning.py and parallel.DataParallelStep._optimizer_step look for this attribute)
    rebuilds_derived_state = True

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, amsgrad=False, maximize=False, capturable=False,
                 differentiable=False):
        if not hasattr(model, "optimizer_step"):
            raise TypeError("vsrcap.optim.Adam takes the ControllableCaptioningModel itself (its step is one library call over the "
                            "model's 28 parameters), got %s; a parameter list goes to torch.optim.Adam" % type(model).__name__)
        for name, on in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable)):
            if on:
                raise ValueError("vsrcap.optim.Adam does not implement %s=True (torch.optim.Adam does)" % name)
        if torch.is_tensor(lr):
            raise ValueError("vsrcap.optim.Adam takes lr as a Python float (a tensor lr is torch's capturable path)")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        self.model = model
        named = dict(model.named_parameters())
        self._keys = [k for _, k in _lib.WEIGHT_FIELDS]
        if sorted(named) != sorted(self._keys):
            raise ValueError("the model's parameters are not the 28 tensors of the library's weight table")
        self._params = [named[k] for k in self._keys]
        for k, p in zip(self._keys, self._params):
            if p.device.type != "cuda":
                raise RuntimeError("vsrcap.optim.Adam steps on the GPU only: parameter %s is on %s (move the model first)" % (k, p.device))
            if p.dtype != torch.float32:
                raise RuntimeError("parameter %s is %s: the library's weights are fp32" % (k, p.dtype))
        # torch's own keys and defaults, so that a checkpoint of either class loads into the other (fused=True: a torch.optim.Adam that
        # loads this optimizer's checkpoint goes on with torch's fused kernel, the closest relative); the parameters in the order of
        # model.parameters(), which is the order torch.optim.Adam(model.parameters()) numbers them in its state_dict
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=True, decoupled_weight_decay=False)
        super().__init__(list(model.parameters()), defaults)

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("vsrcap.optim.Adam has one parameter group: one set of hyper-parameters goes to the library per step "
                             "(per-group values would need a step per group)")
        super().add_param_group(param_group)

    def _group(self):
        if len(self.param_groups) != 1:
            raise RuntimeError("vsrcap.optim.Adam has one parameter group, found %d" % len(self.param_groups))
        g = self.param_groups[0]
        for name in ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay"):
            if g.get(name):                  # (a loaded checkpoint brings its own group options)
                raise RuntimeError("vsrcap.optim.Adam does not implement %s=True (found in param_groups[0])" % name)
        if torch.is_tensor(g["lr"]):
            raise RuntimeError("vsrcap.optim.Adam takes lr as a Python float, found a tensor in param_groups[0]")
        return g

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self._group()
        named = dict(self.model.named_parameters())
        grads, exp_avg, exp_avg_sq, steps = [], [], [], set()
        for k, p in zip(self._keys, self._params):
            if named.get(k) is not p:
                raise RuntimeError("parameter %s of the model was replaced after this optimizer was built: build a new one" % k)
            if p.device.type != "cuda":
                raise RuntimeError("vsrcap.optim.Adam steps on the GPU only: parameter %s is on %s" % (k, p.device))
            g = p.grad
            if g is not None:
                if g.is_sparse:
                    raise RuntimeError("vsrcap.optim.Adam does not support sparse gradients (parameter %s)" % k)
                if g.dtype != torch.float32 or g.device != p.device:
                    raise RuntimeError("the gradient of %s is %s on %s: fp32 on the parameter's device expected" % (k, g.dtype, g.device))
                if not g.is_contiguous():
                    g = g.contiguous()
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if not torch.is_tensor(st["step"]) or st["step"].is_cuda:
                # a loaded checkpoint's count (a device tensor under torch's fused=True, a number in old checkpoints): kept on the
                # host from here on - reading it must not wait for the device at every step
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
            if g is not None:                # torch: a parameter without a gradient takes no step
                steps.add(float(st["step"]))
            grads.append(g)
            exp_avg.append(st["exp_avg"])
            exp_avg_sq.append(st["exp_avg_sq"])
        if not steps:
            return loss
        if len(steps) != 1:
            # the bias corrections depend on the count: ONE pair goes to the library, never one tensor's values for another's
            raise RuntimeError("the parameters with gradients have taken different numbers of steps (%s): the library applies one "
                               "bias correction per call" % sorted(steps))
        step = int(steps.pop()) + 1
        self.model.optimizer_step(self._params, grads, exp_avg, exp_avg_sq, lr=float(group["lr"]), beta1=float(group["betas"][0]),
                                  beta2=float(group["betas"][1]), eps=float(group["eps"]), weight_decay=float(group["weight_decay"]),
                                  step=step)
        for p, g in zip(self._params, grads):
            if g is not None:
                self.state[p]["step"] += 1
        return loss
