// Batched strided accumulation: the arithmetic of the transposed halo exchange
// (HaloEngine::accumulate, halo.hpp). Where the exchange's copies store a
// neighbour's send slab over a halo slab, its transpose takes a halo slab away
// (the slab becomes zero) and adds it into the owner's send slab. One launch
// takes up to MAX_BATCH Copy3D descriptors, each with its own operation.
//
// The kernels share the copies' plan (igg/copy_plan.hpp: the normalised box and
// the flat / gather / chunk path), so the z slab of a C-ordered field - one
// short row per plane row - takes the one-row-per-lane gather path here too.
#pragma once

#include <cstdint>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "igg/copy.hpp"
#include "igg/copy_plan.hpp"

namespace igg {

// Bit 0: dst is read and added to; bit 1: src is cleared afterwards.
enum class AccumOp : int {
  Add = 1,      // dst += src
  Take = 2,     // dst = src, then src = 0
  AddTake = 3,  // dst += src, then src = 0 (self-periodic: both slabs are in the field)
  Zero = 4,     // dst = 0 (a contiguous slab that was sent in place; src is not read)
};

const char* accum_op_name(AccumOp op);
AccumOp accum_op_from_name(const char* name);

// Element types of the host path; the device kernels take F32 and F64.
enum class AccumType : int { F32 = 0, F64, I8, I16, I32, I64, U8, F16, BF16, C64, C128 };

int accum_elem_bytes(AccumType t);

// src and dst of a descriptor never overlap, except that a Zero descriptor
// carries its slab on both sides (the plan looks at both). Two descriptors of
// one launch never share a cell.
struct Accum3D {
  Copy3D c;
  AccumOp op;
};

// The copies' plan of the box, with vec_bytes also set on the chunk path: 16
// when both sides have unit-stride rows whose starts are all 16-byte aligned
// (a lane then moves 16 bytes per access; a row's tail is done by element).
CopyPlan3 plan_accum3d(const Copy3D& c, int elem_bytes, bool gather);

// Device: enqueue all descriptors (any count, MAX_BATCH per launch, in order)
// on `stream`. No scratch, no atomics: every cell has one writer per launch.
void launch_accum3d(const std::vector<Accum3D>& ops, AccumType type, hipStream_t stream);

// Host: perform them now, one after the other.
void host_accum3d(const std::vector<Accum3D>& ops, AccumType type);

}  // namespace igg
