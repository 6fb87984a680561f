"""Differentiable halo exchange, diffusion step and acoustic step.

``update_halo_`` works in place and autograd does not see it.
``igg.autograd.update_halo(*fields)`` is the same exchange out of place, as a
``torch.autograd.Function``: the forward pass clones the fields and exchanges
the clones' halos, the backward pass applies the transpose of the exchange
(``accumulate_halo_``) to the incoming gradients. One call covers all fields, so
both passes group them in one exchange. Like ``update_halo_`` the call is
collective: every rank runs the forward and the backward pass.

``igg.autograd.diffusion3d(T, Cp, ...)`` is the other factor of a time step of
``Diffusion3D``: the stencil update ``S(T)`` out of place (boundary cells keep
``T``'s values), whose backward pass runs the adjoint kernels
(``ops.stencil.diffusion3d_adjoint_``). ``update_halo(diffusion3d(T, Cp, ...))``
is one differentiable step of the model on any number of ranks.

``igg.autograd.acoustic2d(P, Vx, Vy, ...)`` is the staggered update of
``Acoustic2D`` out of place, ``(P2, Vx2, Vy2)``; its backward pass is one launch
of the adjoint kernel (``ops.stencil.acoustic2d_adjoint_``). The step is linear,
so nothing is saved. ``update_halo(Vx2, Vy2)`` after it makes one differentiable
step of that model on any number of ranks (``P2`` is never exchanged).

``igg.autograd.sample_g(fields, P)`` is ``sample_g`` with a backward pass: its
transpose ``spread_g(..., copies="owner")`` of the incoming gradient into
zeros, so a loss on sampled values reaches the fields.
"""
from __future__ import annotations

import torch

from torch.autograd.function import once_differentiable

from .ops import stencil as _stencil
from .parallel.accumulate import accumulate_halo_
from .parallel.halo import update_halo_
from .parallel.sample_g import sample_g as _sample_g
from .parallel.spread_g import spread_g as _spread_g


class _UpdateHalo(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *fields):
        outs = tuple(A.detach().clone() for A in fields)  # (clone keeps a dense field's layout)
        update_halo_(*outs)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        # incoming gradients may be views or expanded: accumulate dense copies of them
        gs = tuple(g.clone(memory_format=torch.contiguous_format) for g in grads)
        accumulate_halo_(*gs)
        return gs


def update_halo(*fields):
    """The fields with their halos updated, as new tensors; differentiable.

    Returns one tensor for one field, a tuple for several. The gradient with
    respect to a field is ``accumulate_halo_`` of the gradient with respect to
    the result: what the result's halo cells received flows back to the cells
    of the rank they were copied from."""
    outs = _UpdateHalo.apply(*fields)
    return outs[0] if len(fields) == 1 else outs


class _Diffusion3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, T, Cp, lam, dt, dx, dy, dz):
        Td = T.detach().contiguous()
        Cpd = Cp.detach().contiguous()
        out = Td.clone(memory_format=torch.contiguous_format)  # boundary cells: T's
        if Td.dim() != 3 or min(Td.shape) >= 3:  # (below 3 there is no interior: S is the identity)
            _stencil.diffusion3d_(out, Td, Cpd, lam=lam, dt=dt, dx=dx, dy=dy, dz=dz)
        ctx.kw = dict(lam=lam, dt=dt, dx=dx, dy=dy, dz=dz)
        # the transpose with respect to T needs no forward state (S is linear in T)
        if ctx.needs_input_grad[1]:
            ctx.save_for_backward(Cpd, Td)
        else:
            ctx.save_for_backward(Cpd)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        Cp = ctx.saved_tensors[0]
        g = gout.contiguous()
        need_t, need_cp = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gT = torch.empty_like(g) if need_t else None
        gCp = torch.empty_like(g) if need_cp else None
        if need_t or need_cp:
            _stencil.diffusion3d_adjoint_(gT, g, Cp, T=ctx.saved_tensors[1] if need_cp else None, gCp=gCp, **ctx.kw)
        return gT, gCp, None, None, None, None, None


def diffusion3d(T, Cp, *, lam: float, dt: float, dx: float, dy: float, dz: float):
    """One diffusion update of ``T`` as a new tensor; differentiable in ``T``
    and ``Cp``.

    The result is ``T + dt*lam/Cp * laplace(T)`` on interior cells, computed by
    ``ops.stencil.diffusion3d_``, and ``T`` itself on boundary cells - the map
    a step of ``Diffusion3D`` applies before its halo exchange. The backward
    pass launches only the adjoint kernels that the inputs requiring a
    gradient ask for (``ops.stencil.diffusion3d_adjoint_``); ``T`` is kept for
    it only when ``Cp`` requires a gradient. CPU and GPU tensors, float32 and
    float64, 3-D; ``lam``, ``dt`` and the spacings are plain numbers."""
    return _Diffusion3D.apply(T, Cp, float(lam), float(dt), float(dx), float(dy), float(dz))


class _Acoustic2D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, Vx, Vy, dt, K, rho, dx, dy):
        ins = [A.detach().contiguous() for A in (P, Vx, Vy)]
        outs = [torch.empty_like(A) for A in ins]
        _stencil._acoustic_step(*outs, *ins, dt=dt, K=K, rho=rho, dx=dx, dy=dy)
        ctx.kw = dict(dt=dt, K=K, rho=rho, dx=dx, dy=dy)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, gP2, gVx2, gVy2):
        if not any(ctx.needs_input_grad[:3]):
            return (None,) * 8
        gin = [g.contiguous() for g in (gP2, gVx2, gVy2)]
        gout = [torch.empty_like(g) for g in gin]
        _stencil.acoustic2d_adjoint_(*gout, *gin, **ctx.kw)
        return tuple(g if need else None for g, need in zip(gout, ctx.needs_input_grad[:3])) + (None,) * 5


def acoustic2d(P, Vx, Vy, *, dt: float, K: float, rho: float, dx: float, dy: float):
    """One staggered acoustic update as new tensors ``(P2, Vx2, Vy2)``;
    differentiable in ``P``, ``Vx`` and ``Vy``.

    The forward pass is the step of ``Acoustic2D`` before its halo exchange
    (``P`` (nx, ny), ``Vx`` (nx+1, ny), ``Vy`` (nx, ny+1); the boundary faces
    of ``Vx``/``Vy`` are copied). The backward pass is one launch of the
    adjoint kernel (``ops.stencil.acoustic2d_adjoint_``); the step is linear,
    so no forward state is kept, and an input that needs no gradient gets
    ``None``. CPU and GPU tensors, float32 and float64; ``dt``, ``K``, ``rho``
    and the spacings are plain numbers (no gradient flows to them)."""
    return _Acoustic2D.apply(P, Vx, Vy, float(dt), float(K), float(rho), float(dx), float(dy))


class _SampleG(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, single, *fields):
        fs = tuple(A.detach() for A in fields)
        ctx.P, ctx.single = P.detach(), single
        ctx.like = [(A.shape, A.dtype, A.device, A.stride()) for A in fs]
        return _sample_g(fs[0] if single else fs, ctx.P)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        g = gout.to(torch.float64).contiguous()
        grads = []
        for k, ((shape, dtype, device, stride), need) in enumerate(zip(ctx.like, ctx.needs_input_grad[2:])):
            if not need:
                grads.append(None)
                continue
            gA = torch.zeros(shape, dtype=dtype, device=device)
            _spread_g(gA, ctx.P, g if ctx.single else g[k], copies="owner")
            grads.append(gA)
        return (None, None, *grads)


def sample_g(fields, P):
    """``sample_g(fields, P)`` (collective, identical on every rank);
    differentiable in the fields, float32 or float64.

    The gradient with respect to a field is ``spread_g`` of the incoming
    gradient into zeros with ``copies="owner"``, in the field's dtype: the
    exact transpose of the interpolation this rank did, so only the owner of a
    point's cell receives, in the cells it read. There is no gradient for
    ``P``. Convention: the incoming gradient is the same on every rank, as for
    a loss that every rank computes from the (replicated) sampled values; the
    per-rank gradients then add up over the ranks to the gradient of that one
    loss. What belongs to another rank's copy of a cell is brought home by the
    ``accumulate_halo_`` that ``adjoint_run`` and ``igg.autograd.update_halo``
    already begin their backward pass with."""
    single = isinstance(fields, torch.Tensor)
    fs = (fields,) if single else tuple(fields)
    return _SampleG.apply(P, single, *fs)
