"""Differentiable halo exchange.

``update_halo_`` works in place and autograd does not see it.
``igg.autograd.update_halo(*fields)`` is the same exchange out of place, as a
``torch.autograd.Function``: the forward pass clones the fields and exchanges
the clones' halos, the backward pass applies the transpose of the exchange
(``accumulate_halo_``) to the incoming gradients. One call covers all fields, so
both passes group them in one exchange. Like ``update_halo_`` the call is
collective: every rank runs the forward and the backward pass.
"""
from __future__ import annotations

import torch

from .parallel.accumulate import accumulate_halo_
from .parallel.halo import update_halo_


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
