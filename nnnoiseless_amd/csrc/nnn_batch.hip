// nnn_batch.hip -- host side of the batched process_frame backend: the state slab in HBM, the
// frame-group kernel pipeline (five stages, six launches per group, spread over a few HIP streams for long calls), parity taps,
// per-kernel timing.
// C ABI declared in include/nnn_batch.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/nnn_batch.h"
#include "../../include/nnn_train.h"
#include "nnn_back.hip"
#include "nnn_model.h"

using namespace nnn;

// One file per concern, in dependency order: each part's header says what it needs from the parts above it.
#include "nnn_batch_core.hip"
#include "nnn_batch_streams.hip"
#include "nnn_batch_floor.hip"
#include "nnn_batch_link.hip"
#include "nnn_batch_launch.hip"
#include "nnn_batch_create.hip"
#include "nnn_batch_snapshot.hip"
#include "nnn_batch_host.hip"
#include "nnn_batch_split.hip"
#include "nnn_batch_vad.hip"
#include "nnn_batch_network.hip"
#include "nnn_batch_debug.hip"
#include "nnn_rate.hip"
#include "nnn_pack.hip"
#include "nnn_train.hip"
#include "nnn_sim.hip"
#include "nnn_fit.hip"
#include "nnn_score.hip"
#include "nnn_gate.hip"
#include "nnn_mix.hip"
#include "nnn_pick.hip"
