// nlzm_stream_plan.h -- what the HOST decides when a single stream is opened, with no device in it: how many chunks a launch takes and whether
// the stream gets a second launch set, so that launch k + 1 (and its pre-pass) is queued while launch k is on the device and the frames of launch
// k are coded beside launch k + 1 (nlzm_hip.cpp, stream_step).  Numbers in, two numbers out.  nlzm_hip.cpp (stream_begin) and the CPU harness
// tests/host_sim/stream_plan_sim.cpp include this one text.  Standard library only; compiles with plain g++ -std=c++17.
#pragma once

#include <stdint.h>

namespace nlzm {
namespace stream_plan {

struct Plan {
    uint32_t batch = 0;                             // chunks per launch
    uint32_t depth = 1;                             // launch sets: 1 -- every launch is collected before the next is queued; 2 -- one launch ahead
};

// free_bytes: what the device has free when the stream is opened; table_bytes: what is put aside for the pre-filter table; per_chunk: what the
// per-launch arrays take per chunk of a launch (about 2.3 KB per position); batch: the chunks per launch asked for (>= 1, already at most nchunks).
//   room = 0.6 * free - table.  A launch that does not fit the room is cut down to what fits (where not even one chunk fits, the batch stays:
//   the allocation says what is wrong).
//   A second launch set is counted like the first: depth 2 where two uncut launches fit the room -- and only where the stream has more chunks
//   than a launch, since nothing is queued across calls and a stream of one launch never has a successor to queue.
inline Plan make_plan(double free_bytes, double table_bytes, double per_chunk, uint32_t batch, uint32_t nchunks)
{
    Plan P;
    P.batch = batch < 1 ? 1u : batch;
    const double room = 0.6 * free_bytes - table_bytes;
    const bool cut = room > per_chunk && (double)P.batch * per_chunk > room;
    if (cut) P.batch = (uint32_t)(room / per_chunk);
    P.depth = !cut && nchunks > P.batch && 2.0 * (double)P.batch * per_chunk <= room ? 2u : 1u;
    return P;
}

}  // namespace stream_plan
}  // namespace nlzm
