// Stub for the reference's brain-engine.h (it needs the Metal host API): what
// the reference's functional-dataset.h relies on that header to have included.
#pragma once
#include <cstdint>
#include <functional>
