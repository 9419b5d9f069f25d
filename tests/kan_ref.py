"""fp64 restatement of the B-spline KAN weight generators (HamGNN_pre.use_kan) for the tests: the forward of one KANLinear / KAN, the expanded rows Phi
the HIP kernel writes, and a helper that turns an `oracle.hamgnn_ref` module into its use_kan form by replacing the weight generators after construction
(the oracle refuses use_kan only in its backbones' config check).  TEST INFRASTRUCTURE: nothing here is imported by the product.

Math (one KANLinear; k = 3, G grid intervals, nb = G + 3 bases on the feature's own G + 7 knots t_0 < .. < t_{G+6}):
    B_{j,0}(x) = [t_j <= x < t_{j+1}],     B_{j,k}(x) = (x - t_j) / (t_{j+k} - t_j) B_{j,k-1}(x) + (t_{j+k+1} - x) / (t_{j+k+1} - t_{j+1}) B_{j+1,k-1}(x)
    y_o = sum_i [ silu(x_i) base_weight[o, i] + sum_j B_{j,3}(x_i) spline_weight[o, i, j] spline_scaler[o, i] ]
No 1/sqrt(fan_in), no activation between layers."""
import numpy as np
import torch
from torch import nn

SPLINE_ORDER = 3
GRID_SIZE, GRID_RANGE = 3, (-1.0, 1.0)


def b_splines(x: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    """x [E, in], grid [in, G + 7] -> [E, in, G + 3]"""
    x = x.unsqueeze(-1)
    t = grid.unsqueeze(0)
    b = ((x >= t[..., :-1]) & (x < t[..., 1:])).to(x.dtype)
    for k in range(1, SPLINE_ORDER + 1):
        left = (x - t[..., :-(k + 1)]) / (t[..., k:-1] - t[..., :-(k + 1)])
        right = (t[..., k + 1:] - x) / (t[..., k + 1:] - t[..., 1:-k])
        b = left * b[..., :-1] + right * b[..., 1:]
    return b


def phi(x: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    """[E, 1 + nb, in]: plane 0 = silu(x), plane 1 + j = B_j(x)"""
    return torch.cat([torch.nn.functional.silu(x).unsqueeze(1), b_splines(x, grid).permute(0, 2, 1)], 1)


class KANLinearRef(nn.Module):
    def __init__(self, h_in, h_out, grid_size=GRID_SIZE, grid_range=GRID_RANGE, generator=None):
        super().__init__()
        step = (grid_range[1] - grid_range[0]) / grid_size
        self.register_buffer("grid", (torch.arange(-SPLINE_ORDER, grid_size + SPLINE_ORDER + 1, dtype=torch.float64) * step + grid_range[0])
                             .expand(h_in, -1).contiguous())
        u = lambda *s: torch.rand(*s, generator=generator, dtype=torch.float64) * 2 - 1
        bound = 1.0 / np.sqrt(h_in)
        self.base_weight = nn.Parameter(u(h_out, h_in) * bound)
        self.spline_weight = nn.Parameter(u(h_out, h_in, grid_size + SPLINE_ORDER) * (0.05 / grid_size))
        self.spline_scaler = nn.Parameter(u(h_out, h_in) * bound)

    def wprime(self) -> torch.Tensor:
        """[1 + nb, in, out]"""
        return torch.cat([self.base_weight.t().unsqueeze(0), (self.spline_weight * self.spline_scaler.unsqueeze(-1)).permute(2, 1, 0)], 0)

    def forward(self, x):
        return torch.einsum("epi,pio->eo", phi(x.to(torch.float64), self.grid.double()), self.wprime().double())


class KANRef(nn.Module):
    """KAN(layers_hidden): the reference's state-dict names `layers.{i}.{grid, base_weight, spline_weight, spline_scaler}`"""

    def __init__(self, hs, grid_size=GRID_SIZE, grid_range=GRID_RANGE, generator=None):
        super().__init__()
        self.hs = list(hs)
        self.layers = nn.ModuleList([KANLinearRef(a, b, grid_size, grid_range, generator) for a, b in zip(hs, hs[1:])])

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return x

    def layer_inputs(self, x):
        """the fp64 input of every layer (the last one's is h_last)"""
        xs = []
        for layer in self.layers:
            xs.append(x.to(torch.float64))
            x = layer(x)
        return xs

    def features(self, x) -> torch.Tensor:
        """Phi [E, (1 + nb) h_pad] fp64 as csrc/kan.hip lays it out: plane p of channel c at column p h_pad + c, padding channels 0"""
        h = self.layer_inputs(x)[-1]
        f = phi(h, self.layers[-1].grid.double())
        E, NP, hl = f.shape
        hp = (hl + 15) // 16 * 16
        out = torch.zeros(E, NP, hp, dtype=torch.float64)
        out[:, :, :hl] = f
        return out.reshape(E, NP * hp)

    def scale_(self, factor):
        """multiply every layer's base_weight and spline_scaler: spreads the inner layers' inputs over the whole grid and beyond"""
        with torch.no_grad():
            for layer in self.layers:
                layer.base_weight.mul_(factor)
                layer.spline_scaler.mul_(factor)
        return self


def regions(x: torch.Tensor, grid: torch.Tensor) -> np.ndarray:
    """histogram of the inputs of one layer over the G + 2 k + 3 regions of their feature's knots: left of the grid, the G + 2 k knot intervals, right of it"""
    idx = (x.double().unsqueeze(-1) >= grid.double().unsqueeze(0)).sum(-1)          # 0 .. G + 7
    return np.bincount(idx.reshape(-1).numpy(), minlength=grid.shape[1] + 1)


def swap_generators(module: nn.Module, seed=0, grid_size=GRID_SIZE, scale=None) -> nn.Module:
    """every `*weight_generator*` FullyConnectedNet of an oracle module replaced by a KANRef of the same layer widths (fp64, seeded)"""
    g = torch.Generator().manual_seed(1000 + seed)
    for parent in list(module.modules()):
        for name, child in list(parent.named_children()):
            if "weight_generator" in name and hasattr(child, "hs"):
                k = KANRef(child.hs, grid_size, generator=g)
                if scale is not None:
                    k.scale_(scale)
                setattr(parent, name, k)
    return module


def state_dict_np(module: nn.Module) -> dict:
    return {k: v.detach().cpu().numpy() for k, v in module.state_dict().items()}
