"""``accumulate_halo_`` — the transpose (adjoint) of ``update_halo_``.

``update_halo_`` copies an owner's values outward into the neighbours' halo
cells; ``accumulate_halo_`` brings what the ranks wrote into their halo cells
home: every halo slab that has a neighbour is added into the owner's matching
send slab and becomes zero. With ``H`` the (linear) map ``update_halo_``
applies to the concatenation of all ranks' local arrays, this is ``Hᵀ``:
``Σ_ranks <H x, y> == Σ_ranks <x, Hᵀ y>``.

Uses: the backward pass of a distributed stencil (``igg.autograd.update_halo``
is the differentiable exchange built on it), adjoint-state computations, and
assembly - particle deposits or flux contributions written into halo cells
that belong to a neighbour.

The data path is ``HaloEngine::accumulate`` (csrc/halo.cpp): dimensions
z -> y -> x, per dimension at most one take launch, one transport phase and one
add launch for all fields and both sides (csrc/kernels/accum_kernels.hip). A
cell gets at most one addend per side and dimension, the left neighbour's
first, without atomics: the result is reproducible bit for bit and the GPU's
equals the CPU's.
"""
from __future__ import annotations

import torch

from .._native import PROC_NULL, IGGError
from . import grid as _grid
from . import halo as _halo

# dtypes the host path adds (every torch dtype with an addition, bool excepted)
HOST_DTYPES = {
    torch.float32: "float32", torch.float64: "float64", torch.int8: "int8", torch.int16: "int16",
    torch.int32: "int32", torch.int64: "int64", torch.uint8: "uint8", torch.float16: "float16",
    torch.bfloat16: "bfloat16", torch.complex64: "complex64", torch.complex128: "complex128",
}
DEVICE_DTYPES = (torch.float32, torch.float64)


def _dim_has_neighbors(gg, d: int) -> bool:
    return bool((gg.neighbors[:, d] != PROC_NULL).any())


def check_accumulate(*fields) -> str:
    """The checks ``accumulate_halo_`` adds to ``update_halo_``'s; returns the
    native name of the element type."""
    gg = _grid.global_grid()
    dtype = fields[0].dtype
    if dtype == torch.bool:
        raise IGGError("accumulate_halo_: bool fields have no addition; use an integer or floating-point type.")
    if fields[0].is_cuda and dtype not in DEVICE_DTYPES:
        raise IGGError(f"accumulate_halo_: GPU fields must be float32 or float64 (got {dtype}); "
                       "the other types are accumulated on the CPU only.")
    if dtype not in HOST_DTYPES:
        raise IGGError(f"accumulate_halo_: fields of type {dtype} cannot be accumulated.")
    for i, A in enumerate(fields):
        for d in range(A.dim()):
            o = _halo._ol(gg, d, A)
            if o >= 2 and _dim_has_neighbors(gg, d) and int(A.shape[d]) < o + int(gg.halowidths[d]):
                raise IGGError(
                    f"The field at position {i + 1} is too small in dimension {d + 1} to accumulate its halo: "
                    f"size(A,dim)={int(A.shape[d])} < ol(A,dim)+halowidths[dim]={o + int(gg.halowidths[d])}, "
                    "a send range would overlap a halo.")
    return HOST_DTYPES[dtype]


def _device_transport(gg):
    """The transport of the device messages: the one ``gather_g`` uses (RCCL;
    host-staged where ranks share a GPU or with IGG_TRANSPORT=staged), also
    when ``update_halo_`` runs over put. Collective on first use."""
    if gg.nprocs == 1 or gg.comm is None:
        return None
    from .gather_g import _device_transport as pick

    return pick(gg.comm)


def accumulate_halo_(*fields) -> None:
    """Add the halo of the given field(s) into the cells of the ranks that own
    them and set it to zero: the transpose of ``update_halo_(*fields)``.

    Dimensions run z, y, x. In each, every halo slab ``[0, w)`` / ``[n-w, n)``
    that has a neighbour is sent to that neighbour and zeroed, and what arrives
    from the left / right neighbour is added into the send slab
    ``[ol-w, ol)`` / ``[n-ol, n-ol+w)`` - the left message first where the two
    share planes (``n < 2*ol``). A side without a neighbour is untouched; a
    dimension whose two neighbours are this rank is done locally.

    Arguments are checked like ``update_halo_``'s; in addition a field needs
    ``n >= ol + w`` in every dimension with neighbours, GPU fields must be
    float32 or float64, and CPU fields may have any type torch adds (not
    bool). Nothing is written or sent when a check fails. Group fields in one
    call: every dimension then takes the same few launches and one transport
    phase for all of them. GPU work is stream-ordered on the current stream;
    the call can be captured in a hipGraph on a single-process grid and over
    RCCL, after one eager call with the same fields.

    ``accumulate_halo_`` followed by ``update_halo_`` gives every copy of a
    cell the sum of all copies where ``overlap == 2*halowidth``."""
    _grid.check_initialized()
    if not fields:
        return
    p = _halo._plan(fields)  # update_halo_'s checks, and the converted field set
    fs, device = p[0], p[1]
    name = check_accumulate(*fields)
    if _halo.loopback_active():
        raise IGGError("accumulate_halo_: the loopback emulation has no transposed exchange; "
                       "use a periodic single-process grid or several ranks.")
    gg = _grid.global_grid()
    transport = None
    stream = 0
    if device:
        stream = torch.cuda.current_stream().cuda_stream
        transport = _device_transport(gg)
        if transport is not None and torch.cuda.is_current_stream_capturing() \
                and transport.name not in _halo.CAPTURABLE:
            raise IGGError(f"accumulate_halo_: the '{transport.name}' transport synchronises with the host and "
                           "cannot be captured in a hipGraph; run eager calls")
    _halo.engine().accumulate_set(fs, name, stream, transport)
    _halo._buf_dtype[device] = fields[0].dtype
