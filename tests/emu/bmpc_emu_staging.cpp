// tests/emu/bmpc_emu_staging.cpp -- TEST INFRASTRUCTURE: the library's stage_layout (csrc/bmpc_host_staging.hpp: how the arrays of a
// synchronous host entry share one device block) as host clang compiles it, in a small shared library of its own.
#include <cstdint>
#include <vector>

#include "../../biped_mpc_py_amd/csrc/bmpc_host_staging.hpp"

using namespace bmpc_host;

// stage_layout on n rows: present[i] != 0 and bytes[i] in, off[i] out (all ones: the row is reported absent).  Returns the bytes
// of the block.
extern "C" uint64_t bmpc_emu_stage_layout(const uint8_t* present, const uint64_t* bytes, int n, uint64_t* off) {
  std::vector<StageRow> rows((size_t)n);
  std::vector<size_t> o((size_t)n);
  for (int i = 0; i < n; ++i) rows[i] = {present[i] != 0, (size_t)bytes[i]};
  const size_t total = stage_layout(rows.data(), rows.size(), o.data());
  for (int i = 0; i < n; ++i) off[i] = o[i] == STAGE_ABSENT ? ~(uint64_t)0 : (uint64_t)o[i];
  return total;
}
