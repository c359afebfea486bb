// Stand-in: HIP ships cooperative groups under its own name.
#pragma once
#include <hip/hip_cooperative_groups.h>
