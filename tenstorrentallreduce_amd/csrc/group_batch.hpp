// group_batch.hpp — a bucket list turned into grouped launches: the one host loop behind every
// launcher of the grouped family (kernels.hip, shard_f32_kernels.hip, adamw_kernels.hip,
// mx_kernels.hip).  The contract:
//   - the buckets are taken in list order; `add` says of each whether it joins the pending launch
//     (it then fills its GroupIn and its entry `slot` of the caller's side table) or was routed by
//     `add` itself, in `own` launches, at its place in the list — the pending members are NOT
//     flushed for it, they go out when their launch is full or the list ends;
//   - a launch is enqueued when member number CAP is reached and at the end of the list;
//   - `launch` gets the GroupSpan, the grid (`grid_of` of the launch's tiles), the index of this
//     grouped launch in the call and the tiles of the grouped launches before it;
//   - the side table is zeroed (Side{}) after every launch;
//   - dry: `launch` is never called (`add` routes nothing either: it knows dry) and the number of
//     launches, the own routes' included, is returned in place of a status;
//   - the first non-OK status, of add, of group_span_make or of launch, ends the walk and is returned.
// No heap: GroupIn[CAP] is on the stack.  Plain C++: the kernel files include it under hipcc,
// tests/test_group_batch.py under g++.
#pragma once

#include <cstdint>

#include "allred.h"
#include "group_span.hpp"

namespace tsa {

// what `add` says of bucket i
struct BatchAdd {
    int status;    // not ALLRED_OK: the walk ends here
    int own;       // < 0: member `slot` of the pending launch, `in` filled; else routed by add, in `own` launches
    GroupIn in;
    static BatchAdd member(const GroupIn& g) { return BatchAdd{ALLRED_OK, -1, g}; }
    static BatchAdd routed(int status, int launches) { return BatchAdd{status, launches, GroupIn{}}; }
    static BatchAdd error(int status) { return BatchAdd{status, 0, GroupIn{}}; }
};

// add(i, slot) -> BatchAdd; grid_of(tiles) -> unsigned; launch(span, grid, index, tile_off) -> status
template <int CAP, class Side, class Add, class GridOf, class Launch>
int group_batch(int count, bool dry, Side& side, Add&& add, GridOf&& grid_of, Launch&& launch) {
    static_assert(CAP >= 1 && CAP <= kGroupMax, "GroupSpan's table holds a launch");
    GroupIn in[CAP];
    int pending = 0, launches = 0, index = 0;
    uint64_t pending_tiles = 0, launched_tiles = 0;
    auto flush = [&]() -> int {
        if (!pending) return ALLRED_OK;
        ++launches;
        const int members = pending;
        const uint64_t tiles = pending_tiles;
        pending = 0;
        pending_tiles = 0;
        if (dry) return ALLRED_OK;
        const unsigned grid = grid_of(tiles);
        GroupSpan span;
        if (!group_span_make(&span, in, members, grid)) return ALLRED_ERR_ARG;
        const int s = launch(span, grid, index++, launched_tiles);
        launched_tiles += tiles;   // a checked list's tiles are below 2^31
        side = Side{};
        return s;
    };
    for (int i = 0; i < count; ++i) {
        const BatchAdd a = add(i, pending);
        int s = a.status;
        if (s == ALLRED_OK && a.own < 0) {
            in[pending++] = a.in;
            pending_tiles += a.in.tiles;
            if (pending == CAP) s = flush();
        } else {
            launches += a.own;
        }
        if (s != ALLRED_OK) return s;
    }
    const int s = flush();
    if (s != ALLRED_OK) return s;
    return dry ? launches : ALLRED_OK;
}

}  // namespace tsa
