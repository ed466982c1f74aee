// crc64_device.h -- the five CRC-64 names tests/emu/lane_emu.cpp used up to the
// revision before the two widths were merged into crc_device.h, so that an
// earlier test tree still builds against this library.  Host emulation only, not
// a device interface; nothing in this tree includes it.
#pragma once

#include "crc_device.h"

namespace lzgpu {

constexpr uint32_t kCrc64Chunk = kCrcChunk;
typedef CrcTables<uint64_t> Crc64Tables;
constexpr auto crc64_make_tables = crc_make_tables<uint64_t>;
constexpr auto crc64_chunk = crc_chunk<uint64_t>;
constexpr auto crc64_fold = crc_fold<uint64_t>;

}  // namespace lzgpu
