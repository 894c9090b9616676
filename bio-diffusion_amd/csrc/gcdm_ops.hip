// libgcdm_ops.so -- the module-level operators (forward + backward) behind plug point 3, the non-production configurations and the
// training objective, the fused message layer and the fused stand-alone GCP2 for training, the fused training update, the EGNN property
// classifier, the fused diffusion objective, and the flat gradient bucket of data-parallel / accumulated training steps.  One translation unit, independent of libgcdm_hip.so (the fused sampling path); C ABI in
// include/gcdm_ops.h, include/gcdm_mp_train.h, include/gcdm_mp_tile.h (the same layer on per-GCP tile kernels), include/gcdm_gcp2_train.h, include/gcdm_optim.h, include/gcdm_classifier.h,
// include/gcdm_objective.h, include/gcdm_grad_bucket.h, include/gcdm_data.h (the device-resident data set: batches, property histograms, context
// draws), include/gcdm_geom.h (the GEOM-Drugs conformer file segmented, split and sorted on the device), include/gcdm_molgraph.h (validity, fragments and graph keys of molecules), include/gcdm_molproc.h (the sanitize and largest-fragment filters of generated molecules), include/gcdm_classifier_train.h (the classifier's column-split first edge layer, forward and backward), include/gcdm_egnn_dynamics.h (the layers of the EGNN dynamics network, forward only) and include/gcdm_matrix_mode.h (the fp32 / bf16x6 switch of the GEMM kernels).  gcdm_ops.tile.hip.h comes first:
// the MFMA tile body, the GEMM launches and the helpers the operator headers share; those depend on it and on gcdm_ops.hip.h's status
// macros, not on each other.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -o bio-diffusion_amd/libgcdm_ops.so bio-diffusion_amd/csrc/gcdm_ops.hip
#include "gcdm_ops.tile.hip.h"
#include "gcdm_ops.hip.h"
#include "../../include/gcdm_ops.h"
#include "gcdm_ops.mp_train.hip.h"
#include "../../include/gcdm_mp_train.h"
#include "gcdm_ops.mp_tile.hip.h"
#include "../../include/gcdm_mp_tile.h"
#include "../../include/gcdm_gcp2_train.h"
#include "gcdm_ops.gcp2.hip.h"
#include "../../include/gcdm_optim.h"
#include "gcdm_ops.optim.hip.h"
#include "../../include/gcdm_grad_bucket.h"
#include "gcdm_ops.bucket.hip.h"
#include "../../include/gcdm_classifier.h"
#include "gcdm_ops.classifier.hip.h"
#include "../../include/gcdm_objective.h"
#include "gcdm_ops.objective.hip.h"
#include "../../include/gcdm_data.h"
#include "gcdm_ops.data.hip.h"
#include "../../include/gcdm_geom.h"
#include "gcdm_ops.geom.hip.h"
#include "../../include/gcdm_molgraph.h"
#include "gcdm_ops.molgraph.hip.h"
#include "../../include/gcdm_molproc.h"
#include "gcdm_ops.molproc.hip.h"
#include "../../include/gcdm_classifier_train.h"
#include "gcdm_ops.classifier_train.hip.h"
#include "../../include/gcdm_egnn_dynamics.h"
#include "gcdm_ops.egnn_dynamics.hip.h"
#include "../../include/gcdm_egnn_train.h"
#include "gcdm_ops.egnn_train.hip.h"
