// gsr_dispatch.h -- how a launcher picks a kernel instantiation from run-time flags: a picker functor with one
// `template <bool...> operator()` that names the kernel (and maps away the combinations that must not exist),
// and dispatch_bools, which calls it with the flags as template arguments.  Exactly the forms the picker can
// return are instantiated.
#pragma once

namespace gsr {

// Run-time booleans into template arguments: f.template operator()<B...>() with B the given values, in order.
template <bool... B, class F>
static auto dispatch_bools(F f) { return f.template operator()<B...>(); }
template <bool... B, class F, class... R>
static auto dispatch_bools(F f, bool b, R... rest) {
    return b ? dispatch_bools<B..., true>(f, rest...) : dispatch_bools<B..., false>(f, rest...);
}

}  // namespace gsr
