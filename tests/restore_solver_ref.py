"""Independent restatement of DDNM on the DPM-Solver++(2M) chain: every step of tests/dpm_solver_ref.py's
solver takes, in place of its clipped x0, that x0's DDNM projection x0' onto {A x0 = y} for A = M o pool_n
(tests/restore_masked_ref.project), and keeps x0' as its history.  Nothing else: the grid, lambda, h and r of each step are
dpm_solver_ref's own, in its direct form; the projection is restore_masked_ref's, a select wherever nothing is measured, so y there
(NaN included) reaches no result.

step() is the library's linear form in fp32 with per-sample coefficients, what the lone op is held to bit for bit."""
import torch

import dpm_solver_ref as DR
import restore_masked_ref as RM


def step(x, eps, h, y, mk, n, cr, crm1, c1, c2, c3):
    """(x_prev, the new history) of one step, fp32, coefficients [B]; h is the history going in."""
    col = lambda v: v.reshape(-1, 1, 1, 1)
    x0 = (col(cr) * x - col(crm1) * eps).clamp(-1, 1)
    x0p = RM.project(x0, y, mk, n)
    return (col(c1) * x0p + col(c2) * x) + col(c3) * h, x0p


def masked_chain(base_betas, spec):
    """restore_masked_ref's chain (ancestral / DDIM) on dpm_solver_ref's grid for `spec`, log-SNR specs included: what order 1
    is compared against."""
    import spaced_ref as SR
    c = RM.RestoreMasked.__new__(RM.RestoreMasked)
    c.sd = SR.SpacedDiffusion(base_betas, set(DR.timesteps(base_betas, spec)))
    c.K = c.sd.num_timesteps
    return c


class RestoreSolver:
    def __init__(self, base_betas, spec, order=2):
        self.solver = DR.DPMSolver(base_betas, spec, order)
        self.K = self.solver.K
        self.timestep_map = self.solver.timestep_map

    def run(self, eps_model, x, y, mk, n):
        """x: x_T [B, C, H, W]; y [B, C, H/n, W/n]; mk [B, H/n, W/n] or None (every block measured).  Returns x after steps K-1 .. 0."""
        s = self.solver
        hist = []
        with torch.no_grad():
            for k in range(self.K - 1, -1, -1):
                x0, _ = s.sd._pred_xstart(eps_model, x, k)
                x0 = RM.project(x0, y, mk, n)
                x = s.step(x, x0, hist, k)
                hist.append(x0)
        return x
