/*
 * alipmpc_sens_obs.h — extension of the C ABI of libalipmpc.so (alipmpc.h, which includes this header): the plan's
 * sensitivities to the obstacles.  Conventions, error codes and alipmpc_cfg are alipmpc.h's.
 */
#ifndef ALIPMPC_SENS_OBS_H
#define ALIPMPC_SENS_OBS_H

#include "alipmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * alipmpc_solve_sens_batch with the third group of inputs: the plan's sensitivities to the obstacles, from the same KKT
 * system with one more right-hand side per obstacle parameter.  The same convention: the barrier
 * parameter, the obstacle selection, leg parity and the detour (whether it fires, and to which side) are held fixed;
 * the detour goal does not depend continuously on the obstacles, so there is no chain rule here.
 *   Inputs and the outputs u_out .. iters as alipmpc_solve_batch (that call's bits); dfoot, du and sens_ok as
 *   alipmpc_solve_sens_batch (that call's bits), any of them may be NULL here.
 *   dfoot_obs B x 3 x P    d foot_out / d obstacle parameter (required), P = alipmpc_sens_obs_cols(cfg)
 *                          = 3 nc_max + 5 ne_max
 *   du_obs    B x 5N x P   d u_out / d obstacle parameter (may be NULL)
 * Columns follow the caller's input slots (not the slots select_obs compacts them into): circle slot j is columns
 * 3 j + (0: cx, 1: cy, 2: r), ellipse slot j columns 3 nc_max + 5 j + (0: cx, 1: cy, 2: a, 3: b, 4: phi); r, a and b
 * are the inflated values as passed.  A slot at or above nc[b] / ne[b], and for modi a slot select_obs dropped, has
 * columns of exactly 0.0.  An instance that is invalid under alipmpc_solve_sens_batch's rule has NaN in every column.
 * One launch of the work-queue form for every B.  The domain of alipmpc_solve_sens_batch (anything else:
 * ALIPMPC_EUNSUPPORTED); P = 0 or dfoot_obs == NULL: ALIPMPC_EINVAL.  Host / device pointers as alipmpc_solve_batch.
 */
int32_t alipmpc_sens_obs_cols(const alipmpc_cfg* cfg);
int alipmpc_solve_sens_obs_batch(void* handle, int64_t B,
                                 const double* x0, const double* goal, const int8_t* leg,
                                 const double* cir, const int32_t* nc,
                                 const double* elp, const int32_t* ne,
                                 const double* u0, const double* last_u,
                                 double* u_out, double* foot_out, double* x_pred,
                                 int32_t* status, int32_t* iters,
                                 double* dfoot, double* du, int32_t* sens_ok,
                                 double* dfoot_obs, double* du_obs,
                                 void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* ALIPMPC_SENS_OBS_H */
