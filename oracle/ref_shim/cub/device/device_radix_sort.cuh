// Stand-in: DeviceRadixSort comes with cub/cub.cuh.
#pragma once
#include <cub/cub.cuh>
