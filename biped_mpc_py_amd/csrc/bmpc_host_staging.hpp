// bmpc_host_staging.hpp -- host only: how the arrays of one synchronous host entry share ONE device block (bmpc_capi.hip: the
// handle's host_in and host_out; rule and helpers there).  Pure arithmetic, stated once for libbmpc.so and for the emulation
// library of tests/emu, which hands it to the tests.
#ifndef BMPC_HOST_STAGING_HPP
#define BMPC_HOST_STAGING_HPP

#include <cstddef>

namespace bmpc_host {

// Every slice starts on the boundary a hipMalloc of its own would give it: no kernel sees a pointer less aligned than one into a
// separate buffer (the solve kernels load their inputs as float4).
constexpr size_t STAGE_ALIGN = 256;
constexpr size_t STAGE_ABSENT = ~(size_t)0;

struct StageRow { bool present; size_t bytes; };

// off[i]: the byte offset of row i in the block -- rows in table order, each present one on a STAGE_ALIGN boundary and clear of
// the next -- or STAGE_ABSENT for a row that is not there: it takes no room.  Returns the bytes of the block (a multiple of
// STAGE_ALIGN; 0 with no row present).
constexpr size_t stage_layout(const StageRow* rows, size_t n, size_t* off) {
  size_t at = 0;
  for (size_t i = 0; i < n; ++i) {
    off[i] = rows[i].present ? at : STAGE_ABSENT;
    if (rows[i].present) at = (at + rows[i].bytes + STAGE_ALIGN - 1) / STAGE_ALIGN * STAGE_ALIGN;
  }
  return at;
}

}  // namespace bmpc_host

#endif
