// capi.hip — host side of the C ABI declared in include/wgsparkl_hip.h: the index of its parts.
//
// Host-language note: the reference's host code is Rust (src/pipeline.rs); this
// image has no Rust toolchain, so the host side above the C ABI is C++ here and
// the Rust shim a maintainer would add is shown in INTEGRATION.md / rust/.
//
// One wgs_data owns one HIP stream and every device buffer of a simulation
// (MpmData owns every wgpu buffer, src/pipeline.rs:84-95). wgs_step only
// enqueues; nothing on the step path synchronises with the host.
//
// This stays ONE translation unit: all kernels land in one code object, in the order in which the parts below define
// or first launch them (placement alone moves a kernel by a few percent). Keep the order of the includes.
#include "../../include/wgsparkl_hip.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <climits>
#include <cstdint>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "kernels_bodies.h"
#include "kernels_cdf.h"
#include "kernels_rigid.h"
#include "kernels_shard.h"
#include "kernels_sort.h"
#include "kernels_transfer.h"
#include "kernels_arrivals.h"

using namespace wgs;

#include "host_state.h"          // error reporting, the handle structs, the owners of device and pinned memory, events, the stream
#include "host_grid.inc"         // the arrays sized by the block capacity, growth, the host's looks at the counters
#include "kernels_readback.h"    // device code of the readers and of the checkpoint / render hand-off
#include "host_substep.inc"      // launch ladders, launch plans, the stages of a substep (begin_substep ... enqueue_finish)
#include "capi_io.inc"           // extern "C": setters and readers (in front of wgs_step: k_export_records keeps its place)
#include "capi_lifecycle.inc"    // the stages of data creation (create_impl drives them); extern "C": create / destroy, wgs_step, wgs_sync
#include "host_sharded.inc"      // RCCL binding and the phases of a sharded substep
#include "capi_sharded.inc"      // the loan of a lockstep group's streams; extern "C": communicators, wgs_shard_attach, the sharded steps
#include "kernels_diag.h"        // device-side diagnostics and their launch sequence
#include "capi_debug.inc"        // extern "C": diagnostics, test hooks, WGS_ABLATE profile readers
#include "kernels_fluid.h"       // WGS_MODEL_FLUID: the kernel of the model switch (last: nothing that existed changes its place)
#include "kernels_models.h"      // per-particle models: the kernels of wgs_set_particle_models / wgs_read_particle_models (behind it, likewise)
#include "kernels_probe.h"       // Eulerian field output: the sampler and the window scatter (behind them, likewise) ...
#include "capi_probe.inc"        // ... extern "C": wgs_sample_grid[_device], wgs_read_grid_window[_device]
#include "kernels_fields.h"      // Lagrangian field output: per-particle stress and strain (behind them, likewise) ...
#include "capi_fields.inc"       // ... extern "C": wgs_read_particle_fields[_device]
#include "kernels_walls.h"       // domain walls: the projection of the wall nodes' velocities (behind them, likewise) ...
#include "capi_walls.inc"        // ... its launch (enqueue_finish reaches it by declaration) and extern "C": wgs_set / wgs_get_domain_walls
#include "capi_plasticity.inc"   // the plasticity rule: the snow instantiations of the fused G2P, the field read-out and the energy passes (behind
                                 // them, likewise; their launch sites reach them by declaration) and extern "C": wgs_set / wgs_get_plasticity_model
#include "kernels_forces.h"      // force fields: the rule on the nodes' velocities (behind every kernel that existed, likewise) ...
#include "capi_forces.inc"       // ... its launch (enqueue_finish reaches it by declaration) and extern "C": wgs_set / wgs_get_force_fields
#include "kernels_emit.h"        // particles added at run time: the device twin of creation's packing, k_append and k_emit (behind them, likewise) ...
#include "capi_emit.inc"         // ... fire_emitters (wgs_step reaches it by declaration) and extern "C": wgs_data_create_reserved, wgs_add_particles, the emitters
#include "kernels_remove.h"      // particles removed at run time: mark, the keep-scan, the compaction (behind them, likewise) ...
#include "capi_remove.inc"       // ... fire_sinks (wgs_step reaches it by declaration) and extern "C": wgs_remove_particles[_device / _in], the sinks
