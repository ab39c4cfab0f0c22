// hades252.hip -- the one translation unit of libhades252 (gfx950 only): arithmetic headers, constant tables, the kernel
// headers by domain (kernels_*.hpp) and, below, launch policy + the C ABI of include/hades252.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <pthread.h>
#include <sched.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/hades252.h"
#include "fr32.hpp"
#include "hades_constants.inc"
#include "hades_literal.hpp"
#include "staging.hpp"
#include "hades_fast.hpp"
#include "k_perm_fast.hpp"
#include "hades_coop.hpp"
#include "hades_lanes.hpp"

using namespace hades;

#include "device_tables.hpp"
#include "kernels_perm.hpp"
#include "kernels_merkle.hpp"
#include "kernels_sponge.hpp"
#include "kernels_cipher.hpp"
#include "kernels_safe.hpp"
#include "kernels_grind.hpp"
#include "hades_inverse_constants.inc"
#include "kernels_inverse.hpp"
#include "kernels_matrix.hpp"
#include "kernels_matrix_stream.hpp"
#include "kernels_mmcs.hpp"
#include "kernels_dmmcs.hpp"
#include "kernels_rowmajor.hpp"
#include "kernels_wmmcs.hpp"
#include "kernels_witness.hpp"
#include "kernels_aux.hpp"


// ------------------------------------------------------------------------------------------
// host side: launch policy and the C ABI of include/hades252.h, by domain (one translation unit: -fno-gpu-rdc)
// ------------------------------------------------------------------------------------------
#include "host_fault.hpp"
#include "launch.hpp"
#include "abi_perm.hpp"
#include "abi_merkle.hpp"
#include "abi_sponge.hpp"
#include "abi_cipher.hpp"
#include "abi_safe.hpp"
#include "abi_witness.hpp"
#include "abi_util.hpp"
#include "host_pin.hpp"
#include "host_pool.hpp"
#include "host_pipe.hpp"
#include "host_callers.hpp"
#include "host_safe.hpp"
#include "host_grind.hpp"
#include "host_inverse.hpp"
#include "host_matrix.hpp"
#include "host_matrix_stream.hpp"
#include "host_mmcs.hpp"
#include "abi_dmmcs.hpp"
#include "abi_rowmajor.hpp"
#include "host_rowmajor.hpp"
#include "abi_wmmcs.hpp"
#include "host_cipher.hpp"
