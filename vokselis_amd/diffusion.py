"""The request and the result of the steady-state diffusion pass (vk_steady_diffusion): Context.steady_diffusion is built on these."""
import math

from . import _native as N

AXES = {"x": 0, "y": 1, "z": 2}


def axis_index(axis) -> int:
    """0, 1, 2 from "x", "y", "z" or from the number itself."""
    if isinstance(axis, str):
        if axis not in AXES:
            raise ValueError("axis: 'x', 'y' or 'z' (or 0, 1, 2)")
        return AXES[axis]
    if isinstance(axis, bool) or int(axis) != axis or not 0 <= int(axis) <= 2:
        raise ValueError("axis: 'x', 'y' or 'z' (or 0, 1, 2)")
    return int(axis)


def auto_omega(n_a: int) -> float:
    """The automatic over-relaxation factor for an extent n_a along the axis, as the library forms it (in double, before its rounding to float)."""
    return 2.0 / (1.0 + 3.141592653589793 / float(n_a + 1))


def diffusion_request(lo, hi=float("inf"), axis="z", spacing=(1, 1, 1), omega: float = 0.0, check_every: int = 32, delta_tol: float = 1e-5, flux_tol: float = 1e-3,
                      max_sweeps: int = 20000, gain: float = 0.0, fill_out: float = 0.0, box=None, install: bool = False) -> N.VkDiffusionRequest:
    """A VkDiffusionRequest.  axis: "x", "y", "z" or 0, 1, 2; spacing: three integers 1 .. DIST_MAX_SPACING (x, y, z); omega: 0 asks for the
    automatic factor, else inside (0, 2); check_every: 1 .. DIFF_MAX_CHECK_EVERY sweeps between two looks at the stopping rule;
    max_sweeps >= check_every; delta_tol, flux_tol: finite, >= 0; gain: 0 asks for 1.  Raises ValueError for what cannot be put into the
    struct or can never be valid; the library refuses the rest."""
    spacing = tuple(spacing)
    if len(spacing) != 3 or any(int(s) != s or not 1 <= int(s) <= N.DIST_MAX_SPACING for s in spacing):
        raise ValueError("spacing: three integers 1 .. DIST_MAX_SPACING (x, y, z)")
    omega = float(omega)
    if not (omega == 0.0 or 0.0 < omega < 2.0):
        raise ValueError("omega: 0 (automatic), or inside (0, 2)")
    if isinstance(check_every, bool) or int(check_every) != check_every or not 1 <= int(check_every) <= N.DIFF_MAX_CHECK_EVERY:
        raise ValueError("check_every: an integer 1 .. DIFF_MAX_CHECK_EVERY")
    if isinstance(max_sweeps, bool) or int(max_sweeps) != max_sweeps or not int(check_every) <= int(max_sweeps) < 2 ** 32:
        raise ValueError("max_sweeps: an integer >= check_every")
    delta_tol, flux_tol, gain, fill_out = float(delta_tol), float(flux_tol), float(gain), float(fill_out)
    if not (math.isfinite(delta_tol) and delta_tol >= 0.0 and math.isfinite(flux_tol) and flux_tol >= 0.0):
        raise ValueError("delta_tol, flux_tol: finite and >= 0")
    if not (math.isfinite(gain) and math.isfinite(fill_out)):
        raise ValueError("gain, fill_out: finite")
    req = N.VkDiffusionRequest()
    req.lo, req.hi, req.omega, req.delta_tol, req.flux_tol, req.gain, req.fill_out = float(lo), float(hi), omega, delta_tol, flux_tol, gain, fill_out
    req.axis = axis_index(axis)
    req.flags = (N.DIFF_CLIP_BOX if isinstance(box, str) and box == "clip" else 0) | (N.DIFF_INSTALL if install else 0)
    req.spacing[0], req.spacing[1], req.spacing[2] = (int(s) for s in spacing)
    req.check_every, req.max_sweeps = int(check_every), int(max_sweeps)
    return req


class Diffusion:
    """The result of Context.steady_diffusion.  The raw fields -- n_foreground, n_inlet, n_outlet, n_box, sweeps, converged, delta, Fin_q,
    Fout_q, sum_c_q, omega, gain -- and what the header derives from them, in double: flux_in, flux_out and flux (their mean, in units of
    D0 * pitch), flux_mismatch (|in - out| over their mean), porosity, effective_diffusivity (D_eff / D0 = flux n_a / (n_b n_c)),
    tortuosity_factor (porosity / (D_eff / D0), inf when the flux is 0) and mean_concentration; where asked for, c (float32 [nz, ny, nx],
    NaN off the set) and dense (the stored map [nz, ny, nx]).  axis (0, 1, 2) and extent (the box's extents x, y, z) are the request's."""

    def __init__(self, res: N.VkDiffusionResult, axis=2, extent=(1, 1, 1), c=None, dense=None):
        for name in ("n_foreground", "n_inlet", "n_outlet", "n_box", "sweeps", "Fin_q", "Fout_q", "sum_c_q"):
            setattr(self, name, int(getattr(res, name)))
        self.converged = bool(res.converged)
        self.delta, self.omega, self.gain = float(res.delta), float(res.omega), float(res.gain)
        self.axis, self.extent = axis_index(axis), tuple(int(e) for e in extent)
        fi, fo = float(self.Fin_q), float(self.Fout_q)
        self.flux_in, self.flux_out = fi / 1073741824.0, fo / 1073741824.0
        self.flux = (fi + fo) / 2147483648.0
        mean = 0.5 * (fi + fo)
        self.flux_mismatch = abs(fi - fo) / abs(mean) if mean != 0.0 else (math.inf if fi != fo else 0.0)
        self.porosity = self.n_foreground / self.n_box if self.n_box else 0.0
        a = self.axis
        cross = float(self.extent[(a + 1) % 3]) * float(self.extent[(a + 2) % 3])
        self.effective_diffusivity = self.flux * float(self.extent[a]) / cross if cross > 0.0 else 0.0
        self.tortuosity_factor = self.porosity / self.effective_diffusivity if self.effective_diffusivity > 0.0 else math.inf
        self.mean_concentration = self.sum_c_q / (1073741824.0 * self.n_foreground) if self.n_foreground else 0.0
        self.c, self.dense = c, dense

    def __repr__(self):
        return "Diffusion(n_foreground=%d, porosity=%.6g, sweeps=%d, converged=%s, flux=%.6g, effective_diffusivity=%.6g, tortuosity_factor=%.6g)" % (
            self.n_foreground, self.porosity, self.sweeps, self.converged, self.flux, self.effective_diffusivity, self.tortuosity_factor)
