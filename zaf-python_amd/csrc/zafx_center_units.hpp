// zafx_center_units.hpp -- the name this header had before the two unit cutters became one: everything is in zafx_units.hpp.
#pragma once
#include "zafx_units.hpp"
