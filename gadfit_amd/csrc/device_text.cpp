// device_text.cpp -- embeds the files of device/ (device_text.h).  #embed is a C23 / C++26 directive that this compiler
// accepts in C++17 (-Wno-c23-extensions); it resolves relative to this file.
#include "device_text.h"

namespace gfh {

const char kExp[] = {
#embed "device/exp.hip"
, 0};
const char kPowLn[] = {
#embed "device/pow_ln.hip"
, 0};
const char kParsBlock[] = {
#embed "device/pars_block.hip"
, 0};
const char kUnseen[] = {
#embed "device/unseen.hip"
, 0};
const char kSweep[] = {
#embed "device/sweep.hip"
, 0};
const char kWaveSum[] = {
#embed "device/wave_sum.hip"
, 0};
const char kFusedSweepGram[] = {
#embed "device/fused_sweep_gram.hip"
, 0};
const char kChi2[] = {
#embed "device/chi2.hip"
, 0};
const char kOmega[] = {
#embed "device/omega.hip"
, 0};
const char kOmegaJt[] = {
#embed "device/omega_jt.hip"
, 0};
const char kBatchWgSum[] = {
#embed "device/batch_wg_sum.hip"
, 0};
const char kBatchCube[] = {
#embed "device/batch_cube.hip"
, 0};
const char kBatchFit[] = {
#embed "device/batch_fit.hip"
, 0};
const char kBatchFitKernels[] = {
#embed "device/batch_fit_kernels.hip"
, 0};
const char kBatchFitBounded[] = {
#embed "device/batch_fit_bounded.hip"
, 0};
const char kBatchCov[] = {
#embed "device/batch_cov.hip"
, 0};
const char kBatchEval[] = {
#embed "device/batch_eval.hip"
, 0};
const char kEval[] = {
#embed "device/eval.hip"
, 0};

}  // namespace gfh
