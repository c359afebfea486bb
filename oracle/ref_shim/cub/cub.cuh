// Stand-in: hipCUB under the name cub.
#pragma once
#include <hipcub/hipcub.hpp>
namespace cub = hipcub;
