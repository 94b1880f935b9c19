"""Independent restatement of RePaint (Lugmayr et al., CVPR 2022) for the inpainting tests.

Nothing here imports models.diffusion.respace.  The schedule is RePaint's get_schedule_jump as a list of states walked pairwise
(a decreasing pair is a reverse step at the first state, an increasing pair a single forward step), over the respaced DDPM of
spaced_ref.SpacedDiffusion.  A run of j forward steps is folded into one draw of q(x_{s+j} | x_s) whose coefficients are built
by composing the j single steps x <- sqrt(1 - beta) x + sqrt(beta) z in float64 (mean factor times sqrt(alpha), variance times alpha
plus beta), which is how the product states its jump: the same distribution as RePaint's j draws, one draw instead of j.

Each reverse op (row k = N - 1 - op index) is: the clipped-x0 ancestral step with draw z1, the known image noised to the op's output
level with draw z2, a select on the mask, then the folded jump with draw z3 where the op has one.  The draws come from
oracle/philox_ref with keys (seed, step = k, stream, stream | 2^30, stream | 2^29) in NHWC element order.  The eps model runs at the
trained timestep map[tau]."""
import math

import numpy as np
import torch

import spaced_ref as SR
from oracle import philox_ref as PR


def get_schedule_jump(t_T, jump_length, jump_n_sample):
    """RePaint's scheduler.get_schedule_jump (n_sample = 1, no start resampling): the states visited, ending in -1."""
    jumps = {}
    for j in range(0, t_T - jump_length, jump_length):
        jumps[j] = jump_n_sample - 1
    t = t_T
    ts = []
    while t >= 1:
        t = t - 1
        ts.append(t)
        if jumps.get(t, 0) > 0:
            jumps[t] = jumps[t] - 1
            for _ in range(jump_length):
                t = t + 1
                ts.append(t)
    ts.append(-1)
    return ts


def ops_from_pairs(t_T, jump_length, jump_n_sample):
    """(tau of each reverse op, forward steps that follow it) from the pairwise walk over get_schedule_jump."""
    ts = get_schedule_jump(t_T, jump_length, jump_n_sample)
    taus, fwd = [], []
    for t_last, t_cur in zip(ts[:-1], ts[1:]):
        if t_cur < t_last:
            taus.append(t_last)
            fwd.append(0)
        else:
            assert t_cur == t_last + 1
            fwd[-1] += 1
    return taus, fwd


def draw(shape_nchw, seed, k, stream):
    b, c, h, w = shape_nchw
    z = PR.philox_normal(b * h * w * c, seed, k, stream).reshape(b, h, w, c)
    return torch.from_numpy(np.ascontiguousarray(z.transpose(0, 3, 1, 2)))


class RePaint:
    def __init__(self, base_betas, spec, jump_length, jump_n_sample):
        T = len(base_betas)
        use = set(range(T)) if spec is None else SR.space_timesteps(T, spec)
        self.sd = SR.SpacedDiffusion(base_betas, use)
        self.K = self.sd.num_timesteps
        self.taus, self.fwd = ops_from_pairs(self.K, jump_length, jump_n_sample)
        self.N = len(self.taus)

    def _ab(self, s):
        return 1.0 if s < 0 else float(self.sd.alphas_cumprod[s])

    def _fold(self, s, j):
        """float64 (mean factor, std) of j single forward steps from state s."""
        a, v = 1.0, 0.0
        for i in range(s + 1, s + j + 1):
            beta = 1.0 - self._ab(i) / self._ab(i - 1)
            a, v = a * math.sqrt(1.0 - beta), v * (1.0 - beta) + beta
        return a, math.sqrt(v)

    def run(self, eps_model, x, known, mask, seed, stream=0):
        """x: x_T [B, C, H, W]; known / mask of the same shape (mask 1 = known).  Returns x after all N ops."""
        f32 = lambda v: torch.tensor(v, dtype=torch.float64).float()
        shape = tuple(x.shape)
        known = torch.where(mask != 0, known, torch.zeros_like(known))
        with torch.no_grad():
            for op, (tau, j) in enumerate(zip(self.taus, self.fwd)):
                k = self.N - 1 - op
                x_unk = self.sd.p_sample(eps_model, x, tau, draw(shape, seed, k, stream))
                ab = self._ab(tau - 1)
                x_kn = f32(math.sqrt(ab)) * known + f32(math.sqrt(1.0 - ab)) * draw(shape, seed, k, stream | (1 << 30))
                x = torch.where(mask != 0, x_kn, x_unk)
                if j:
                    a, b = self._fold(tau - 1, j)
                    x = f32(a) * x + f32(b) * draw(shape, seed, k, stream | (1 << 29))
        return x
