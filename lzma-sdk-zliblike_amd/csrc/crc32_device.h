// crc32_device.h -- CRC-32 is crc_device.h with its default register type.  Named
// by tests/emu up to the revision before the two widths were merged; it stays so
// that an earlier test tree still builds.  Nothing in this tree includes it.
#pragma once

#include "crc_device.h"
