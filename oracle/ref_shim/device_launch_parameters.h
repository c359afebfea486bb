// Stand-in for the CUDA header of this name: the HIP runtime declares the same API.
#pragma once
#include <hip/hip_runtime.h>
