"""Field memory of the models: native allocations and carving several fields
out of one of them (docs/COHERENCE.md: fine-grained memory for fields the
neighbours store into; profiles/r2_offsets/: one allocation with gaps)."""
from __future__ import annotations

import torch


def native_buffer(nbytes: int, kind: int, device) -> torch.Tensor:
    """1-D uint8 device tensor of ``nbytes`` in native memory of MemKind
    ``kind`` (csrc/include/igg/ipc.hpp), owned by torch (freed with it)."""
    from torch.utils import dlpack

    from .._native import native

    with torch.cuda.device(device):
        return dlpack.from_dlpack(native.alloc_dlpack(int(nbytes), int(kind)))


def ipc_limit() -> int:
    """Allocation size from which IPC export is refused (csrc/include/igg/ipc.hpp)."""
    from .._native import native

    return int(native.IPC_MAX_BYTES)


def carve(tensors, gap: int = None, kind=None, split_at=None, device=None, split_kind=None):
    """Copies of ``tensors`` placed in one buffer, each ``gap`` bytes after the
    end of the one before (``gap`` None: at the next multiple of 256 bytes).
    ``kind``: None = torch's caching allocator, else a native MemKind (1 =
    fine-grained, 4 = HIP VMM) allocated by the runtime and handed over through
    DLPack. ``split_at``: if the one buffer would reach this many bytes, one
    allocation per tensor instead (the IPC size limit), of MemKind
    ``split_kind`` if given. Meta tensors give shape and dtype only:
    uninitialised views on ``device``."""
    sizes = [t.numel() * t.element_size() for t in tensors]
    pitch = [-(-n // 256) * 256 if gap is None else n + gap for n in sizes]
    total = sum(pitch)
    device = tensors[0].device if device is None else device
    if split_at is not None and total >= split_at and len(tensors) > 1:
        k = kind if split_kind is None else split_kind
        return [carve([t], None if gap is None else 0, k, device=device)[0] for t in tensors]
    if kind is None:
        buf = torch.empty(total, dtype=torch.uint8, device=device)
    else:
        buf = native_buffer(total, kind, device)
    out, pos = [], 0
    for t, n, p in zip(tensors, sizes, pitch):
        v = buf[pos:pos + n].view(t.dtype).view(t.shape)
        if t.device.type != "meta":
            v.copy_(t)
        out.append(v)
        pos += p
    return out
