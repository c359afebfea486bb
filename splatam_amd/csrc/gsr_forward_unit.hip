// gsr_forward_unit.hip -- the forward's stage files compiled as one translation unit, so that their kernels,
// which run back to back in every step (preprocess, column scan, duplicate, render), lie in one code object,
// as they did when they were one file: the library keeps the code objects it was measured with
// (profiles/forward_split_bench.txt).  Each file still stands alone: its own includes, compiles by itself,
// names nothing of the others.  build.FORWARD_STAGES lists them in this order.
#include "gsr_preprocess.hip"
#include "gsr_binning.hip"
#include "gsr_radix.hip"
#include "gsr_forward.hip"
#include "gsr_reuse.hip"
