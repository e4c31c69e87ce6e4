// asr_pending.h -- the one protocol of the count / fill pairs (contract: include/asr_hip.h, "Count / fill pairs").
//
// A _count call parks device pointers into the context's scratch arena for its _fill call.  The context has ONE slot that
// says whose they are and which generation of the arena they point into (Arena::generation, bumped by every reset and
// rewind): a fill is served only while both still hold, so no fill ever walks memory another operator has since been given.
// Plain C++ with no HIP include: tests/pending_protocol.cpp compiles it with the host compiler alone.
#pragma once
#include <cstdint>

enum class PendingOp : int {
    None = 0,
    MultiRadiusSearch,
    DualCells,
    Contour,
    Components,
    MeshSimplify,
    MeshEdges,
    MeshFillHoles,
    PointsMerge,
};

struct Pending {
    PendingOp op = PendingOp::None;
    uint64_t scratch_generation = 0;
};

// first statement of every _count: whatever was pending is void, also when this count fails
static inline void pending_begin(Pending& p) { p.op = PendingOp::None; }
// last statement of a _count that succeeded (the early returns for empty input included)
static inline void pending_commit(Pending& p, PendingOp op, uint64_t scratch_generation) {
    p.op = op;
    p.scratch_generation = scratch_generation;
}
// _fill: true when the most recent successful count was `op`'s and the scratch arena has not been recycled since.  The
// slot is empty afterwards either way: a count is filled once.
static inline bool pending_claim(Pending& p, PendingOp op, uint64_t scratch_generation) {
    const bool ok = op != PendingOp::None && p.op == op && p.scratch_generation == scratch_generation;
    p.op = PendingOp::None;
    return ok;
}
