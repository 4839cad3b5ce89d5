/*
 * bmpc.h -- C ABI of libbmpc.so: batched HECTOR force-and-moment MPC on MI355X (gfx950).
 *
 * Drop-in boundary for the hot path of junhengl/biped_mpc_py (REF = bipedalLocomotionMPC.py):
 * one call solves B independent instances of what REF:187-304 `solve_mpc` solves once.
 * The reference has no FFI of its own (it is one Python file); these entry points are what a
 * ctypes binding replacing the body of `solve_mpc` would call.
 *
 * Conventions: plain C, no torch / HIP types in signatures.  All arrays are row-major and
 * instance-major.  Every function returns 0 on success or a negative bmpc_status code;
 * bmpc_last_error() gives a thread-local message.  A handle owns its device memory and stream;
 * one handle is not thread-safe, distinct handles are.  Per-instance failures (iteration cap,
 * NaN) are reported in status[], never by failing the batch.
 */
#ifndef BMPC_H
#define BMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMPC_ABI_VERSION 13

/* `stream` arguments are hipStream_t values passed as void*.  NULL is HIP's null (legacy default)
 * stream -- what torch.cuda.current_stream().cuda_stream is when no stream context is active -- so a
 * launch is ordered after the caller's earlier work on that stream and before its later work, exactly
 * like a hip* call.  BMPC_STREAM_OWN selects the handle's private (non-blocking) stream: the one bmpc_debug_assemble and the
 * host-pointer low-level entries run on.  bmpc_solve_batch / bmpc_solve_batch_f64 / bmpc_solve_batch_io run their chunks on
 * three prioritised streams of their own, which wait for whatever the handle's own stream held when the call began. */
#define BMPC_STREAM_OWN ((void*)(intptr_t)-1)

enum bmpc_status {
  BMPC_OK = 0,
  BMPC_ERR_INVALID = -1,     /* bad argument (null pointer, B > max_batch, unsupported h ...) */
  BMPC_ERR_NO_DEVICE = -2,   /* no usable HIP device: the library never falls back to the CPU */
  BMPC_ERR_HIP = -3,         /* a HIP runtime call failed */
  BMPC_ERR_ALLOC = -4
};

/* bmpc_params.path: which kernel family solves (REF:203-216 keeps the stage structure that BMPC_PATH_STAGE exploits) */
enum bmpc_path {
  BMPC_PATH_AUTO = 0,
  BMPC_PATH_DENSE = 1,
  BMPC_PATH_STAGE = 2
};

enum bmpc_penalty_mode {
  BMPC_PENALTY_SCALED = 0,
  BMPC_PENALTY_ABSOLUTE = 1
};

/* bmpc_params.rescue */
enum bmpc_rescue_mode {
  BMPC_RESCUE_AUTO = -1,
  BMPC_RESCUE_OFF = 0,
  BMPC_RESCUE_ON = 1
};

/* per-instance status[] values written by the solver */
enum bmpc_instance_status {
  BMPC_SOLVED = 0,           /* stopping criteria met */
  BMPC_MAX_ITER = 1,         /* iteration cap reached (result is the last iterate: iters = max_iter, and iteration max_iter
                                always ends on a stopping test, so residuals[] are its own and the states those of the returned
                                controls).  The stopping criteria are four: (1, 2) the primal and the step residual within
                                eps_pri / eps_dua, (3) no inactive row still pulling (penalty x |z~ - z| <= 1e-6 x 2 min R x
                                max(1, |x|)), (4) the rows of step 0 -- the applied control -- within 5 x max(eps_pri, eps_dua)
                                relative to step 0's own norm (not on the dense kernel of h = 12); an instance that fails only
                                the third re-classifies at once, and one that can no longer re-classify (max_refactor spent, or
                                adapt_every = 0) is accepted without it -- it is never held to the cap by it */
  BMPC_NUMERICAL = 2         /* NaN/Inf encountered */
};

/*
 * Parameter block.  Field names follow the reference's attribute bags:
 *   MPC   (REF:22-32): h, dt, x_cmd, Q, R, kv
 *   Biped (REF:34-48): m, I, lt, lh, g, mu, f_max, f_min, tau_max, tau_min
 * plus the solver's own knobs.  `half` is the gait half period used by the reference-foot
 * generator (REF:101-105 hard-codes 5).  bmpc_default_params() fills the reference defaults.
 */
typedef struct bmpc_params {
  int32_t h;                 /* horizon length (REF:24); supported: see bmpc_supported_horizon */
  int32_t half;              /* gait half period in steps (REF:101: 5) */
  double dt;                 /* REF:25 */
  double kv;                 /* REF:29 */
  double x_cmd[12];          /* REF:26; used when the per-instance x_cmd argument is NULL */
  double Q[13];              /* REF:27 (13th weight acts on the constant state: inert) */
  double R[12];              /* REF:28 */
  double m;                  /* REF:36 */
  double I[9];               /* REF:37-39 body inertia, row-major */
  double lt, lh;             /* REF:40-41 (the 0.01 / 0.02 margins of REF:254-255 are applied inside) */
  double g;                  /* REF:42 */
  double mu;                 /* REF:44; used when the per-instance mu argument is NULL */
  double f_max[3], f_min[3];     /* REF:45-46 */
  double tau_max[3], tau_min[3]; /* REF:47-48 */
  /* solver (ADMM with active-set adaptive penalties) */
  double rho;                /* initial penalty on every row (default 0.03; 0.045 at h >= 20); see penalty_mode */
  double rho_eq_scale;       /* multiplier for rows with l == u (pinned variables) */
  double rho_lo;             /* floor of the per-row penalties */
  double rho_hi_f;           /* ceiling for force-like rows (force box, friction) */
  double rho_hi_m;           /* ceiling for moment-like rows (moment box, line-foot) */
  double kappa;              /* per re-classification a row's penalty moves by this factor: up
                                (towards its ceiling) if the row is active, down (towards rho_lo) if not;
                                damped to sqrt(kappa) after 10 factorisations of an instance, to its
                                fourth root after 16 (rare active-set cycles) */
  double alpha;              /* over-relaxation */
  double eps_pri, eps_dua;   /* relative stopping tolerances */
  int32_t max_iter;          /* iteration cap (default 1000 at h <= 12, else 1500; worst seen at the reference's weights: 240 / 315) */
  int32_t check_every;       /* stopping test period */
  int32_t adapt_start;       /* first penalty re-classification (default 5 at h <= 12, 10 at h = 14 .. 18 and h > 20, 20 at h = 20) */
  int32_t adapt_every;       /* re-classification period (0 = never; default 5 at h <= 12 -- see adapt_early --, 20 at h = 14 .. 20,
                                10 beyond: the period follows the cost of a factorisation relative to an iteration) */
  int32_t max_refactor;      /* cap on re-factorisations per instance (then plain ADMM with the penalties reached); default 60:
                                a decade or two away from the reference's weights 1 instance in ~300 keeps re-classifying
                                for up to 60 rounds (damped moves) and then converges; at the reference's weights <= 18 */
  int32_t warm_adapt_start;  /* first re-classification of a warm-started solve (bmpc_set_warm_start); 0 = adapt_start */
  int32_t path;              /* kernel family: BMPC_PATH_AUTO (default: the faster one for h), BMPC_PATH_DENSE (explicit
                                6h x 6h inverse in registers; h <= 20) or BMPC_PATH_STAGE (stage-structured Riccati solve,
                                O(h) work and state; every supported h).  Same optimum, same outer method. */
  int32_t penalty_mode;      /* BMPC_PENALTY_SCALED (default): rho, rho_lo, rho_hi_*, rho_eq are the values at the reference
                                problem -- REF:22-48 defaults at THIS problem's horizon for h <= 20 (so a fixed model shows
                                no horizon scaling between h = 8 and h = 20: the absolute values were tuned and soaked
                                there), at h = 10 for h > 20 (the stiff end then grows like sum k^2 ~ h^3) -- and are
                                scaled by the curvature of the problem at hand relative to it: stiff end (Q, dt, m, I, h)
                                for the ceilings and rho_eq, 2 R for the floor, their geometric mean for the start.  The
                                ceilings and rho_eq are capped at 1e6 (2 min R + rho_lo) -- 4e5 on the dense family --, what
                                the f32 factors hold.
                                Degenerate curvature scales (every Q of a state group zero) are BMPC_ERR_INVALID, not a
                                silent fallback.  BMPC_PENALTY_ABSOLUTE: the fields are taken as they are.
                                bmpc_effective_penalties() returns what a block resolves to. */
  int32_t rescue;            /* BMPC_RESCUE_AUTO (default), _OFF, _ON: after a solve on the dense family, the instances whose
                                status is not 0 are solved again by the stage family (one more launch on the same stream,
                                its workgroups leave at once where the status is 0; the outputs of a rescued instance,
                                iters / nfactor / residuals included, are those of the second solve).  AUTO: on unless the
                                model and weights are the reference's own (REF:22-48), where the dense family has not
                                lost an instance in 6 M and the launch would only cost ~1 %.  No effect on the stage path. */
  int32_t accel;             /* 1 (default) / 0: secant extrapolation of the iterate at the stopping tests (Anderson acceleration with
                                memory one: w <- T(w) - gamma (T(w) - w), gamma from the last two state changes; two sums in the
                                reduction the stopping test already pays for).  Both families (not the dense kernel of h = 12 nor
                                the stage kernel of h = 22 / 24: no LDS / registers for it): 5-7 % fewer iterations and
                                factorisations up to h = 20, 2-5 % beyond, 1-4 % less kernel time.  Same fixed point. */
  int32_t adapt_early;       /* two-rate re-classification schedule (ABI 10): the first `adapt_early` re-classifications -- the one at
                                adapt_start included -- are `adapt_every` iterations apart, the later ones `adapt_late`.  The active set
                                is found in the first ~20 iterations (45 of 240 rows change class between iterations 10 and 20,
                                < 1 after 40), so early re-classifications are worth a factorisation each and late ones mostly
                                walk a few rows along their ladder.  Default at h <= 12: 5 / 5 / 3 / 20 (iterations 5, 10, 15, 35,
                                55 ...); 0 (or adapt_late = 0): every re-classification adapt_every apart (the schedule of ABI <= 9) */
  int32_t adapt_late;
  int32_t adapt_busy;        /* ... but `adapt_busy` iterations after a (late) re-classification that still found more than `adapt_flips` of
                                the instance's rows in another class than the one before: the instances that keep turning are the
                                tail of a batch and are not made to wait.  0: always adapt_late.  Default at h <= 12: 10, 1.
                                (Ignored -- always adapt_late -- by the kernels that do not count class changes: the dense h = 12
                                kernel, whose reduction has no slot for it, and the five-steps-per-lane stage variant, h = 21 .. 24.) */
  int32_t adapt_flips;
  int32_t confirm_from;      /* confirmation: from re-classification number confirm_from + 1 on, a row found in the SAME class as at the
                                previous re-classification moves by kappa_confirm instead of kappa (>= the length of a ladder: straight
                                to its ceiling / floor) -- a row that turns late otherwise costs three more factorisations walking
                                there.  Default at h <= 12: 3, 400; kappa_confirm = 0: off.  (Ignored by the five-steps-per-lane
                                stage variant, h = 21 .. 24 -- no register for the previous classes; the dense h = 12 kernel DOES
                                confirm: it keeps the classes, it only does not count their changes.) */
  int32_t reserved0;
  double kappa_confirm;
  /* low-level control side of the loop (REF:29-32, 43): used by bmpc_low_level_control* / bmpc_foot_position_world* only */
  double kp[9], kd[9];       /* REF:30-31, row-major 3x3 */
  double swingHeight;        /* REF:32 */
  double hip_offset[3];      /* REF:43 */
} bmpc_params;

typedef struct bmpc_handle_s* bmpc_handle;

/* Library / ABI identification. */
int bmpc_abi_version(void);
const char* bmpc_last_error(void);
/* 1 if a kernel is built for this horizon, else 0: every h in [1, 40] (REF:24: the horizon is a plain field of MPC; odd and
 * short horizons run on the stage-structured family).
 * bmpc_supported_horizon_path(h, path) asks for one kernel family (dense: even h in [8, 20]). */
int bmpc_supported_horizon(int h);
int bmpc_supported_horizon_path(int h, int path);
/* The penalties the kernels will use for this parameter block after the scaling of `penalty_mode`:
 * out5 = {rho, rho_eq, rho_lo, rho_hi_f, rho_hi_m}.  Host arithmetic only (no device needed). */
int bmpc_effective_penalties(const bmpc_params* params, double* out5);
/* The kernel family a handle's solves run on (BMPC_PATH_DENSE or BMPC_PATH_STAGE; <0 on error). */
int bmpc_solver_path(bmpc_handle h);
/* 1 if this handle's solves are followed by the rescue pass (see bmpc_params.rescue), else 0 (<0 on error). */
int bmpc_rescue_enabled(bmpc_handle h);
/* Reference defaults (REF:22-48) and solver defaults for horizon h. */
int bmpc_default_params(bmpc_params* p, int h);

/* Create a solver bound to HIP device `device` for at most max_batch instances per call.
 * Replaces: constructing MPC() / Biped() (REF:475-476) -- the parameters are uploaded once. */
int bmpc_create(bmpc_handle* out, const bmpc_params* params, int device, int max_batch);
int bmpc_destroy(bmpc_handle h);
/* Replace the parameter block (same horizon as at creation). */
int bmpc_set_params(bmpc_handle h, const bmpc_params* params);
int bmpc_get_params(bmpc_handle h, bmpc_params* out);

/*
 * Solve B instances; HOST pointers.  Replaces REF:187-304 solve_mpc for a batch.
 *   x_fb     [B][12]   state feedback (REF:13 ordering: euler, pos, omega_w, v_w)
 *   foot     [B][6]    world foot positions [foot1 xyz, foot2 xyz] (REF:479)
 *   contact  [B][h][2] 0/1 contact schedule (REF:482-484)
 *   phase    [B]       k = int(t // dt) % h (REF:99-100), computed by the caller in fp64
 *   x_cmd    [B][12]   or NULL -> params.x_cmd
 *   mu       [B][h][2] or NULL -> params.mu
 * outputs
 *   controls [B][h][12] row k = [f1 f2 m1 m2] (REF:302)
 *   states   [B][h][13] or NULL; row k = predicted state at step k+1 (REF:301)
 *   iters    [B] or NULL, residuals [B][2] or NULL (primal, step), status [B] or NULL
 *   nfactor  [B] or NULL: factorisations used
 * Synchronous: returns after the results are in the output arrays.
 */
int bmpc_solve_batch(bmpc_handle h, int B,
                     const float* x_fb, const float* foot, const uint8_t* contact,
                     const int32_t* phase, const float* x_cmd, const float* mu,
                     float* controls, float* states,
                     int32_t* iters, float* residuals, int32_t* status, int32_t* nfactor);

/*
 * Same with fp64 outputs -- the dtype REF:300-304 returns (`states`, `controls` are fp64 arrays there) -- so that a caller
 * who needs the reference's dtype does not widen 25 h values per instance in a second pass: the widening happens while the
 * results are unpacked from the pinned staging block, chunk by chunk, overlapped with the solve of the later chunks.  The
 * values are the fp32 results of bmpc_solve_batch, exactly (float -> double is exact).
 *
 * Both host-pointer entries stage through page-locked memory owned by the handle (one packed block in, one packed block per
 * chunk out) and split a batch of >= 1024 instances into up to 3 contiguous chunks (55 / 30 / 15 %) on streams of descending
 * priority: a chunk's device-to-host copy and its unpacking into the caller's pageable arrays overlap the later chunks' solves.  Results do not depend on the chunking (the kernels' arithmetic does not depend on the
 * position in a batch).  With warm start, a dispatch order or the profile buffer set the batch goes out as one chunk.
 * bmpc_last_kernel_ms afterwards: from the start of the first chunk's kernel to the end of the last one's.
 */
int bmpc_solve_batch_f64(bmpc_handle h, int B,
                         const float* x_fb, const float* foot, const uint8_t* contact,
                         const int32_t* phase, const float* x_cmd, const float* mu,
                         double* controls, double* states,
                         int32_t* iters, float* residuals, int32_t* status, int32_t* nfactor);

/*
 * The handle's I/O block (ABI 10): host arrays the caller fills and reads IN PLACE -- what a control loop that keeps its buffers
 * wants, and the fastest way across PCIe.  The block is page-locked host memory owned by the handle and mapped into the device's
 * address space: the inputs cross in ONE copy, and the results arrive in the host arrays already widened to the fp64
 * REF:300-304 returns (the widening happens in the kernels' epilogues; the values are the fp32 results of bmpc_solve_batch,
 * exactly) with no unpacking pass: `controls` and the per-instance counters are stored by the kernels straight into the host
 * arrays, `states` follow by copy engine chunk by chunk (up to 3 chunks on prioritised streams, as in bmpc_solve_batch; the last
 * chunk's states go the way of the controls) -- on MI355X a kernel's own stores into host memory sustain ~8.6 GB/s, the copy
 * engine ~50 GB/s, and a 4096-instance batch returns 8.2 MB in 0.8 ms.
 *   bmpc_host_io(h, B, with_x_cmd, with_mu, with_states, &views)   lays the block out for batches of exactly B instances and
 *       returns the array pointers (layouts as in bmpc_solve_batch; x_cmd / mu / states NULL unless asked for).  The views hold
 *       this layout until the next bmpc_host_io of the handle (another layout re-uses or outgrows the block; the memory behind
 *       an old view is not freed before bmpc_destroy, so a stale view reads stale data, never unmapped memory).
 *   bmpc_solve_batch_io(h, B)   solves what the input views hold; synchronous: on return the output views hold the results.
 * Ordered after whatever the handle's own stream held when the call began (BMPC_STREAM_OWN launches).  Warm start, dispatch
 * order and the rescue pass apply as for bmpc_solve_batch_device (with warm start or a dispatch order: one chunk).
 */
typedef struct bmpc_host_views {
  float* x_fb;        /* [B][12] */
  float* foot;        /* [B][6] */
  uint8_t* contact;   /* [B][h][2] */
  int32_t* phase;     /* [B] */
  float* x_cmd;       /* [B][12] or NULL */
  float* mu;          /* [B][h][2] or NULL */
  double* controls;   /* [B][h][12] */
  double* states;     /* [B][h][13] or NULL */
  int32_t* iters;     /* [B] */
  float* residuals;   /* [B][2] */
  int32_t* status;    /* [B] */
  int32_t* nfactor;   /* [B] */
} bmpc_host_views;
int bmpc_host_io(bmpc_handle h, int B, int with_x_cmd, int with_mu, int with_states, bmpc_host_views* out);
int bmpc_solve_batch_io(bmpc_handle h, int B);
/* Layout generation of the handle's I/O block (ABI 11): a counter that moves with every bmpc_host_io call of the handle that gets
 * past argument validation.  A call rejected there (null handle or views, B out of range, hipSetDevice failing) leaves both the
 * layout and the counter as they were; a call that fails after that point still moves the counter and leaves no layout
 * (bmpc_solve_batch_io then refuses).  A caller that caches the views compares it
 * with the value it read after its own bmpc_host_io: any other layout call in between -- same B, other with_* flags, hence other
 * offsets -- shows, instead of the cached views being trusted.  Returns the counter (>= 0), or a negative error code. */
int bmpc_host_io_generation(bmpc_handle h);

/*
 * Same, DEVICE pointers (memory of the handle's device), asynchronous on `stream`
 * (see BMPC_STREAM_OWN above for NULL and the handle's own stream).  Nothing is copied.
 * This is the entry the bench times and the one a device-resident control loop uses.
 */
int bmpc_solve_batch_device(bmpc_handle h, int B,
                            const float* x_fb, const float* foot, const uint8_t* contact,
                            const int32_t* phase, const float* x_cmd, const float* mu,
                            float* controls, float* states,
                            int32_t* iters, float* residuals, int32_t* status, int32_t* nfactor,
                            void* stream);

/* Block until everything queued on the handle's own stream is done, and the LAST bmpc_solve_batch_device /
 * bmpc_rollout_device solve launch of this handle whatever stream it was given (earlier launches on a caller's
 * stream are the caller's to wait for, with that stream).
 *
 * One stream in flight per handle: a handle owns ONE set of per-solve state -- the warm-start buffer (read at the
 * start of a solve, written at its end), the roll-out scratch, the event pair of bmpc_last_kernel_ms -- and nothing
 * orders two solves of the same handle that run on DIFFERENT streams.  Use one stream per handle at a time (or one
 * handle per stream); solves on one stream are ordered like any other work on it. */
int bmpc_synchronize(bmpc_handle h);

/*
 * Introspection for parity tests of the assembly stage (DEVICE->HOST copy inside).
 * Runs the assembly only and returns, per instance, in fp64:
 *   x_ref [B][h][12] (REF:61-70), foot_ref [B][h][6] (REF:72-109),
 *   Gt [B][6h][6h] wrench-space Hessian, qt [B][6h] wrench-space gradient,
 * any of which may be NULL.
 */
int bmpc_debug_assemble(bmpc_handle h, int B,
                        const float* x_fb, const float* foot, const uint8_t* contact,
                        const int32_t* phase, const float* x_cmd, const float* mu,
                        double* x_ref, double* foot_ref, double* Gt, double* qt);

/*
 * Reference tracking (ABI 12): the inputs of a solve as one named descriptor, with what the solve tracks.  By default the kernels
 * generate the references of REF:61-70 (constant commanded velocities from x_fb) and REF:72-109 (the foothold heuristic); a
 * caller who tracks something else -- stairs, a crouch, a planner's footholds -- supplies them per instance:
 *   x_ref    [B][h][12] or NULL: row j = x_ref[0:12, j] of REF:61-70 (the 13th row of ones is implied)
 *   foot_ref [B][h][6]  or NULL: row j = foot_ref[:, j] of REF:72-109
 * the layouts of bmpc_debug_assemble's outputs, in fp32.  Each is independent of the other; a NULL one is generated exactly as
 * by the ABI-11 entries (which are these entries with both NULL, bit for bit).  A supplied array drives everything the generated
 * one drives: the linearisation of step j (Rot, I_w, R_inv from x_ref[0:3, j], REF:150-164), the lever arms
 * foot_ref[:, j] - x_ref[3:6, j] (REF:174-175) and the cost target of the state after step j (REF:282-284) -- column 0 included,
 * used as given (the generator sets it to x_fb, REF:63).  It does not change the free response (from x_fb), the friction, box and
 * pinned rows, or the body axes of the line-foot rows, which are those of R = eul2rotm(x_fb[0:3]) (REF:193) whatever x_ref
 * holds.  Non-finite references, or a pitch of +-90 degrees (R_inv singular, as in the reference), give that instance
 * status BMPC_NUMERICAL, never a failed batch.  The rescue pass solves against the same references.
 *   bmpc_solve_inputs_f64      bmpc_solve_batch_f64 with the descriptor (host pointers, synchronous, the same chunked path)
 *   bmpc_solve_inputs_device   bmpc_solve_batch_device with the descriptor (device pointers, asynchronous on `stream`)
 *   bmpc_debug_assemble_inputs bmpc_debug_assemble with the descriptor: x_ref / foot_ref return the references used (a supplied
 *                              one widened to fp64), Gt / qt the assembly built from them
 * A NULL handle or descriptor, or foot == NULL without foot_ref, is BMPC_ERR_INVALID.  The handle's I/O block (bmpc_host_io) and
 * bmpc_rollout_device always generate.
 */
typedef struct bmpc_inputs {
  const float* x_fb;        /* [B][12] */
  const float* foot;        /* [B][6]; may be NULL iff foot_ref != NULL (only the foothold generator reads it) */
  const uint8_t* contact;   /* [B][h][2] */
  const int32_t* phase;     /* [B] */
  const float* x_cmd;       /* [B][12] or NULL -> params.x_cmd */
  const float* mu;          /* [B][h][2] or NULL -> params.mu */
  const float* x_ref;       /* [B][h][12] or NULL -> REF:61-70 generated */
  const float* foot_ref;    /* [B][h][6] or NULL -> REF:72-109 generated */
} bmpc_inputs;
int bmpc_solve_inputs_f64(bmpc_handle h, int B, const bmpc_inputs* in,
                          double* controls, double* states,
                          int32_t* iters, float* residuals, int32_t* status, int32_t* nfactor);
int bmpc_solve_inputs_device(bmpc_handle h, int B, const bmpc_inputs* in,
                             float* controls, float* states,
                             int32_t* iters, float* residuals, int32_t* status, int32_t* nfactor,
                             void* stream);
int bmpc_debug_assemble_inputs(bmpc_handle h, int B, const bmpc_inputs* in,
                               double* x_ref, double* foot_ref, double* Gt, double* qt);

/*
 * Evaluation (ABI 13): what the MPC's own model makes of a GIVEN control sequence -- the solver's own (to rank the samples of a
 * batch by the cost REF:278-286 minimises), or a foreign one (a warm-start guess, a policy's output, last period's plan shifted,
 * another solver's answer).  Inputs: the descriptor of a solve (references supplied or generated exactly as a solve generates
 * them) and
 *   controls [B][h][12] fp32, row k = [f1 f2 m1 m2] (REF:302)
 * outputs, per instance, each optional (NULL = not wanted; at least one must be given), fp64:
 *   cost       sum_k (x_{k+1} - x_ref[:, k])' diag(Q) (x_{k+1} - x_ref[:, k]) + u_k' diag(R) u_k over all 13 state entries (the 13th
 *              contributes 0): non-negative, the number to rank samples by
 *   objective  the value the reference hands to its solver, 1/2 z'Pz + q'z with z = [X(U); U] (REF:278-297)
 *              = cost - sum_k sum_i Q_i x_ref[i, k]^2 (i over 13, the row of ones included)
 *   states     [h][13]: row k = the state after step k, x_{k+1} = A_k x_k + B_k u_k, x_0 = [x_fb; 1], A_k / B_k of REF:148-185
 *              linearised about x_ref[:, k], foot_ref[:, k]: X(U) of the equality block REF:203-216 -- what `states` of a solve
 *              is for the solver's own controls (the 13th entry is 1)
 *   violation  [4]: per row class of Aqp z <= bqp (REF:273-274) the largest positive part of Aqp z - bqp, 0 if the class holds:
 *              [0] friction pyramid (REF:220-232; per-step mu honoured), [1] force rows of the box (REF:235-251, both signs,
 *              bounds scaled by `contact`: a swing leg's force counts in full), [2] moment rows of the box, [3] line foot
 *              (REF:254-271: body axes of R = eul2rotm(x_fb[0:3]), REF:193, whatever x_ref holds; margins 0.01 / 0.02)
 * Arithmetic: fp64 throughout, on the fp32 inputs widened (the fp64 controls of bmpc_solve_batch_f64 are fp32 values: narrowing them
 * is exact).  One launch, O(h) work per instance; the result of an instance does not depend on B or on its position in the batch.
 * A non-finite input, control or reference entry, or a reference pitch within fp32 rounding of +-90 degrees (|cos pitch| < 2^-22:
 * R_inv of REF:160-164 is singular there), gives NaN in every output of that instance and touches no other instance.
 *   bmpc_evaluate_device   DEVICE pointers, asynchronous on `stream` (NULL / BMPC_STREAM_OWN as for bmpc_solve_batch_device);
 *                          nothing is copied
 *   bmpc_evaluate          HOST pointers, synchronous (staged through the handle's own stream)
 * A NULL handle, descriptor, `controls` or `out`, all four outputs NULL, foot == NULL without foot_ref, or B outside
 * [0, max_batch] is BMPC_ERR_INVALID; the NULL checks come before a device is touched.  Every supported horizon (1 .. 40), and the
 * same kernel whatever family the handle solves with (`path` plays no part).  The evaluation reads the handle's parameter block
 * (bmpc_set_params takes effect; the solver's own knobs are not used) and none of its per-solve state: the warm-start buffer, the
 * dispatch order, the event pair and the I/O block are left alone, and bmpc_last_kernel_ms keeps reporting the last SOLVE.  Queued
 * behind a bmpc_solve_*_device call on the same stream with that call's `controls` buffer as input, it needs no synchronisation
 * in between.
 */
typedef struct bmpc_eval_out {
  double* cost;        /* [B] or NULL */
  double* objective;   /* [B] or NULL */
  double* states;      /* [B][h][13] or NULL */
  double* violation;   /* [B][4] or NULL: friction, force box, moment box, line foot */
} bmpc_eval_out;
int bmpc_evaluate_device(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls,
                         const bmpc_eval_out* out, void* stream);
int bmpc_evaluate(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const bmpc_eval_out* out);

/*
 * Gradient of the evaluated cost (added under ABI 13; BMPC_ABI_VERSION is unchanged because the addition is purely additive --
 * no existing entry, struct or meaning moves -- so a caller detects it by the symbol, e.g. dlsym(lib, "bmpc_evaluate_grad_device")).
 * `cost` above is an exact quadratic in the controls; its gradient is one adjoint sweep over the horizon, in the same launch shape
 * as the evaluation.  Uses: first-order refinement of a foreign plan, a differentiable MPC cost inside a training loop, the
 * sensitivity of a plan's cost to the measured state, and an optimality check of a solver's answer that needs no multipliers
 * (at an optimum U*, grad_u . (V - U*) >= 0 for every feasible V).  Inputs: those of bmpc_evaluate*.
 * outputs, per instance, each optional (NULL = not wanted; at least one must be given), fp64:
 *   cost     the same value and the same bits as bmpc_evaluate*'s `cost` on the same inputs
 *   grad_u   [h][12]: d cost / d controls, row k = 2 diag(R) u_k + B_k' lambda_k with the costates
 *            lambda_k = d cost / d x_{k+1} = 2 diag(Q) (x_{k+1} - x_ref[:, k]) + A_{k+1}' lambda_{k+1} (nothing above k = h - 1),
 *            A_k / B_k of REF:148-185 as the evaluation linearises them
 *   grad_x0  [12]: d cost / d x_fb THROUGH THE INITIAL CONDITION x_0 = [x_fb; 1] ONLY, A_0' lambda_0.  The references, the lever
 *            arms and the linearisation are held fixed, whether they were supplied or generated: generated references (and the
 *            line-foot body axes, which do not enter the cost) depend on x_fb, and that dependence is deliberately NOT
 *            differentiated.  With supplied references this is the full derivative.
 * The cost is quadratic in the controls, so grad_u(U + D) - grad_u(U) is the Hessian-vector product H D; there is no separate entry.
 * Arithmetic, bad instances (NaN in every output of that instance, no other instance touched), independence of B and of the place
 * in the batch: as for the evaluation.
 *   bmpc_evaluate_grad_device   DEVICE pointers, asynchronous on `stream` (same rules as bmpc_evaluate_device); nothing is copied
 *   bmpc_evaluate_grad          HOST pointers, synchronous (staged through the handle's own stream)
 * A NULL handle, descriptor, `controls` or `out`, all three outputs NULL, foot == NULL without foot_ref, or B outside
 * [0, max_batch] is BMPC_ERR_INVALID; the NULL checks come before a device is touched; B = 0 succeeds.  Every supported horizon
 * (1 .. 40); the handle's kernel family plays no part; the handle's parameter block is read and none of its per-solve state is
 * touched (as for bmpc_evaluate*).  bmpc_eval_out is unchanged.
 */
typedef struct bmpc_grad_out {
  double* cost;        /* [B] or NULL */
  double* grad_u;      /* [B][h][12] or NULL */
  double* grad_x0;     /* [B][12] or NULL */
} bmpc_grad_out;
int bmpc_evaluate_grad_device(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls,
                              const bmpc_grad_out* out, void* stream);
int bmpc_evaluate_grad(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const bmpc_grad_out* out);

/*
 * KKT certificate of given controls (added under ABI 13; BMPC_ABI_VERSION is unchanged because the addition is purely additive, so a
 * caller detects it by the symbol, e.g. dlsym(lib, "bmpc_certify_device")).  Answers, on the device and from the controls alone: is
 * this point the constrained optimum of REF:187-297, how far off is it, and which inequality rows bind at what price.
 * Every inequality row of REF:273-274 touches the controls of one leg at one step, and grad_u above is the gradient of the condensed
 * cost, so stationarity grad_u + C' lam = 0, lam >= 0 splits into 2 h non-negative least-squares problems per instance with 6
 * unknown directions and at most 18 candidate rows each (Lawson-Hanson, fp64, at most 3 x 18 least-squares solves per leg).
 * Inputs: those of bmpc_evaluate*, and `act_tol`: a row with slack = b - C u is ACTIVE iff slack <= act_tol (1 + |b|); only active
 * rows may carry a multiplier (a negative act_tol activates no feasible row).  act_tol must not be NaN.
 * The 36 rows of step k, in the reference's order:  0..7 friction (leg 0 then leg 1, each (+x, +y, -x, -y) - mu z, REF:220-232),
 * 8..19 upper bounds +u <= ub (u = [f1 f2 m1 m2], bounds scaled by contact, REF:235-251), 20..31 lower bounds -u <= -lb,
 * 32..35 line foot (leg 0 then leg 1, REF:254-271).  Row 8k + r of G at REF:273 is friction row r of step k, 8h + 24k + r box row
 * r, 32h + 4k + r line-foot row r.
 * outputs, per instance, each optional (NULL = not wanted; at least one must be given):
 *   lam      [h][36] fp64: the multipliers, >= 0, exactly 0 on rows that are not active.  Unique where the active rows of a leg are
 *            linearly independent; elsewhere (a swing leg pinned at 0, tau_max[0] = 0) one valid choice
 *   resid    [h][12] fp64: grad_u + C' lam, the stationarity residual (unique: the distance of -grad_u to the cone of active rows)
 *   summary  [4] fp64: stationarity = max |resid|; primal_ineq = the largest positive part of C u - b (the maximum of
 *            bmpc_evaluate*'s four `violation` entries, same bits); complementarity = max |lam_i slack_i|; grad_scale = max |grad_u|
 *            (stationarity / grad_scale is the relative figure)
 *   n_active int32: the number of active rows
 *   status   int32: 0 = every least-squares problem converged, 1 = the cap on solves was reached on some leg (lam is still >= 0 and
 *            supported on active rows, so the residuals are valid, only not the smallest), 2 = bad instance
 * Bad instances (as for the evaluation): NaN in every fp64 output, n_active = -1, status = 2; no other instance is touched.
 * Independence of B and of the place in the batch: as for the evaluation.
 *   bmpc_certify_device   DEVICE pointers, asynchronous on `stream` (same rules as bmpc_evaluate_device); nothing is copied
 *   bmpc_certify          HOST pointers, synchronous (staged through the handle's own stream)
 * A NULL handle, descriptor, `controls` or `out`, all five outputs NULL, a NaN act_tol, foot == NULL without foot_ref, or B outside
 * [0, max_batch] is BMPC_ERR_INVALID; the NULL checks come before a device is touched; B = 0 succeeds.  Every supported horizon
 * (1 .. 40); the handle's kernel family plays no part; the handle's parameter block is read and none of its per-solve state is
 * touched.
 */
typedef struct bmpc_cert_out {
  double* lam;         /* [B][h][36] or NULL */
  double* resid;       /* [B][h][12] or NULL */
  double* summary;     /* [B][4] or NULL */
  int32_t* n_active;   /* [B] or NULL */
  int32_t* status;     /* [B] or NULL */
} bmpc_cert_out;
int bmpc_certify_device(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, double act_tol,
                        const bmpc_cert_out* out, void* stream);
int bmpc_certify(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, double act_tol, const bmpc_cert_out* out);

/*
 * S candidate plans per instance in one launch, ranked and blended on the device (added under ABI 13; BMPC_ABI_VERSION is unchanged
 * because the addition is purely additive, so a caller detects it by the symbol, e.g. dlsym(lib, "bmpc_evaluate_samples_device")).
 * What a sampling controller holds is B situations and S candidate plans for each -- a nominal plan plus noise, last period's plan
 * shifted, a policy's proposals.  This operation scores them all, picks the best and forms the softmin-weighted mean plan (the
 * update of MPPI and of predictive sampling) without replicating an input and without leaving the device.  Inputs: those of
 * bmpc_evaluate* for B instances, and
 *   controls [B][S][h][12] fp32: plan s of instance b, row k = [f1 f2 m1 m2]
 *   smp      S, the prices w_viol of the four violation classes and the temperature of the weights (below)
 * Per-sample outputs, each optional (NULL = not wanted; at least one output of the struct must be given), fp64:
 *   cost      [S]     what bmpc_evaluate* returns as `cost` for the inputs of instance b and the controls controls[b][s]: the same
 *   violation [S][4]  arithmetic (fp64 on the widened fp32 inputs; references supplied or generated; per-step mu), likewise
 *   score     [S]     cost + w_viol[0] violation[0] + w_viol[1] violation[1] + w_viol[2] violation[2] + w_viol[3] violation[3],
 *                     added in that order
 * A sample's cost, violation and score depend on nothing but its instance's inputs and its own controls: not on B, S, b or s, nor
 * on how the launch groups the samples.  A sample is VALID iff its score is finite.  A non-finite control entry makes that sample's
 * cost, violation and score NaN and touches no other sample; a bad instance (as for the evaluation: a non-finite input or
 * reference entry, a reference pitch within fp32 rounding of +-90 degrees) makes every sample of it NaN.
 * Per-instance reductions, each optional:
 *   n_valid  int32: the number of valid samples
 *   best     int32: the smallest index among the valid samples of smallest score; -1 if n_valid is 0
 *   weights  [S] fp64: e_s / sum_s e_s with e_s = exp(-(score_s - m) / temperature), m the best score, for valid samples; an invalid
 *            sample has e_s and its weight exactly +0
 *   u_mean   [h][12] fp64: sum_s weights_s controls[b][s], accumulated in fp64; an invalid sample's controls do not enter it
 *   ess      fp64: 1 / sum_s weights_s^2, the effective sample size (1 .. n_valid)
 * If n_valid is 0 the weights are all +0 and u_mean and ess are NaN.  A temperature of +inf gives uniform weights 1 / n_valid.
 * The reduced values of an instance do not depend on B or on its place in the batch and repeat bit for bit from run to run: no
 * floating-point atomics, every sum in an order fixed by (S, h) alone.
 *   bmpc_evaluate_samples_device   DEVICE pointers, asynchronous on `stream` (same rules as bmpc_evaluate_device); nothing is
 *                                  copied.  Two launches on that stream: the per-sample kernel and, where a reduced output is
 *                                  wanted, the reductions behind it.
 *   bmpc_evaluate_samples          HOST pointers, synchronous (staged through the handle's own stream)
 * Checked before a device is touched, each BMPC_ERR_INVALID: a NULL `smp`, S outside [1, 65536], a w_viol entry that is NaN,
 * negative or infinite, a temperature that is NaN or <= 0 (these first); a NULL handle, `in`, `controls` or `out`; all eight outputs
 * NULL; foot == NULL without foot_ref; B outside [0, max_batch].  B = 0 succeeds.  max_batch bounds B, not B S.
 * The handle's parameter block is read (bmpc_set_params takes effect) and none of its per-solve state is touched, as for
 * bmpc_evaluate*: warm start, dispatch order, event pair and I/O block are left alone and bmpc_last_kernel_ms keeps reporting the
 * last SOLVE.  The reductions read the scores and the weights on the device; where the caller asks for a reduced output but not for
 * `score` or `weights`, those live in a scratch buffer owned by the handle and grown on demand.  A bmpc_evaluate_samples_device call
 * that has to GROW that scratch is not asynchronous (the old block is freed, which waits for the device), and calls that use the
 * scratch of one handle must be ordered on one stream; a caller that passes both `score` and `weights` never touches it.
 */
typedef struct bmpc_samples {
  int32_t S;            /* samples per instance, 1 .. 65536 */
  int32_t reserved0;
  double  w_viol[4];    /* finite, >= 0: price of the largest violation per row class (friction, force box, moment box, line foot) */
  double  temperature;  /* > 0, +inf allowed (uniform weights) */
} bmpc_samples;
typedef struct bmpc_samples_out {     /* each NULL = not wanted; at least one non-NULL */
  double*  cost;       /* [B][S]     */
  double*  violation;  /* [B][S][4]  */
  double*  score;      /* [B][S]     */
  int32_t* best;       /* [B]        */
  int32_t* n_valid;    /* [B]        */
  double*  weights;    /* [B][S]     */
  double*  u_mean;     /* [B][h][12] */
  double*  ess;        /* [B]        */
} bmpc_samples_out;
int bmpc_evaluate_samples_device(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const bmpc_samples* smp,
                                 const bmpc_samples_out* out, void* stream);
int bmpc_evaluate_samples(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const bmpc_samples* smp,
                          const bmpc_samples_out* out);

/*
 * The step either side of the MPC solve, batched; HOST pointers, synchronous.
 *   bmpc_foot_position_world  replaces getFootPositionWorld (REF:406-424, with getFootPositionBody REF:367-404):
 *       x_fb [B][12], q [B][10] joint angles  ->  pf_w [B][6]
 *   bmpc_low_level_control    replaces lowLevelControl (REF:444-470, with getLegKinematics REF:306-365 and
 *       swingLegControl REF:426-442):
 *       x_fb [B][12], t [B] (seconds, fp64), pf_w [B][6], q [B][10], qd [B][10],
 *       contact0 [B][2] = contact[0, 0:2], u0 [B][12] = controls[0]  ->  tau [B][10]
 * The *_device variants take DEVICE pointers and a stream (NULL = the null stream, BMPC_STREAM_OWN = the
 * handle's) and do not synchronise.
 */
int bmpc_foot_position_world(bmpc_handle h, int B, const float* x_fb, const float* q, float* pf_w);
int bmpc_foot_position_world_device(bmpc_handle h, int B, const float* x_fb, const float* q, float* pf_w, void* stream);
int bmpc_low_level_control(bmpc_handle h, int B, const float* x_fb, const double* t, const float* pf_w,
                           const float* q, const float* qd, const uint8_t* contact0, const float* u0, float* tau);
int bmpc_low_level_control_device(bmpc_handle h, int B, const float* x_fb, const double* t, const float* pf_w,
                                  const float* q, const float* qd, const uint8_t* contact0, const float* u0,
                                  float* tau, void* stream);

/* Gait scheduler, batched (replaces get_contact_sequence REF:50-59 and the phase index of REF:99-100;
 * SURVEY 8(f) row 2).  phase[b] = int(t[b] // dt) % h in fp64 with Python's float floor division, and
 * contact[b][n][g] = 1 iff leg g is in stance at schedule step k + n:  ((k + n + offset[g]) mod period) < duty[g].
 * bmpc_gait_default(g, half) gives the reference's table generalised to a half period: period = 2 half,
 * offset = {0, half}, duty = {half, half} (half = 5: exactly REF:52-55).  Either output may be NULL.
 * h and dt are the handle's parameters; `contact` has h rows per instance (the reference slices ten rows
 * whatever mpc.h is -- identical for its h = 10). */
typedef struct bmpc_gait {
  int32_t period;
  int32_t offset[2];
  int32_t duty[2];
} bmpc_gait;
int bmpc_gait_default(bmpc_gait* g, int half);
int bmpc_contact_sequence(bmpc_handle h, int B, const double* t, const bmpc_gait* gait, int32_t* phase, uint8_t* contact);
int bmpc_contact_sequence_device(bmpc_handle h, int B, const double* t, const bmpc_gait* gait, int32_t* phase,
                                 uint8_t* contact, void* stream);

/*
 * Receding-horizon use (the reference solves one step, REF:13-17, and lists real-time use as
 * its TODO, README.md:6-7).
 *
 * bmpc_set_warm_start: with enable != 0 every later bmpc_solve_batch* call through this handle leaves the final
 * solver state of each instance (iterate, multipliers, per-row penalties: 48 B per lane) in a device buffer owned
 * by the handle, and starts from the state the previous call left for the same batch index (same B), advanced by
 * `shift` horizon steps (0: the schedule phase did not move; 1: one control period later) and with the penalties
 * pulled back towards their initial value, rho0 (rho / rho0)^theta (theta in [0, 1]; 1 keeps them).  The first
 * call after enabling, after bmpc_reset_warm_start, or with another B starts cold; so does the first call after a
 * bmpc_set_params that moved the handle to the other kernel family (the families keep different states), and an
 * instance whose stored state is not finite (its previous solve failed) -- that instance alone.  The optimum is the
 * same; only the iteration count changes.  enable == 0 switches it off.  A shift outside [0, h) or a theta outside
 * [0, 1] (NaN included) is BMPC_ERR_INVALID, whatever `enable` is, and leaves the previous setting as it was.
 *
 * bmpc_rollout_device: `steps` closed-loop control periods of B instances on one stream, DEVICE pointers, no host
 * arithmetic and no synchronisation: per period  t -> (phase, contact) [bmpc_contact_sequence_device]  ->  solve
 * [bmpc_solve_batch_device]  ->  x_fb <- states[:, 0, 0:12] (the model's own prediction, REF:301), t += dt.
 *   x_fb [B][12] in/out, foot [B][6], t [B] fp64 in/out, gait NULL = the handle's default schedule,
 *   x_cmd [B][12] or NULL, mu [B][h][2] or NULL (constant over the roll-out);
 *   u0_traj [steps][B][12], x_traj [steps][B][12] (state after each period), iters_traj [steps][B],
 *   status_any [B] (OR of the per-period status values): each may be NULL.
 *
 * bmpc_set_dispatch_order: workgroups start in index order and an instance's duration varies (35-105 iterations at
 * h = 10), so the last instances of a batch decide when it ends.  Measured on MI355X (4096 instances): a roll-out
 * spends 3 % less per period with the longest instances first, a plain batch dispatched in its own longest-first order
 * 1-9 % less depending on the box (15 % only when the INPUTS are permuted, tools/order_probe.py: the indirection
 * costs part of it).  The duration cannot be predicted from the inputs, but in a
 * closed loop the previous period's iteration count predicts it: with longest_first_rollouts != 0 (default)
 * bmpc_rollout_device sorts every period's dispatch by the iteration counts of the period before (one small
 * kernel).  order_dev, if non-NULL, is a DEVICE permutation of 0 .. B-1 used by every later solve of this handle
 * (workgroup g solves instance order_dev[g]) and takes precedence; it must stay valid until replaced.  The results
 * never depend on the order.
 */
int bmpc_set_warm_start(bmpc_handle h, int enable, int shift, double theta);
int bmpc_reset_warm_start(bmpc_handle h);
int bmpc_rollout_device(bmpc_handle h, int B, int steps, float* x_fb, const float* foot, double* t,
                        const bmpc_gait* gait, const float* x_cmd, const float* mu,
                        float* u0_traj, float* x_traj, int32_t* iters_traj, int32_t* status_any, void* stream);
int bmpc_set_dispatch_order(bmpc_handle h, const int32_t* order_dev, int longest_first_rollouts);

/*
 * Closed-loop simulation (added under ABI 13; BMPC_ABI_VERSION is unchanged because the addition is purely additive, so a caller
 * detects it by the symbol, e.g. dlsym(lib, "bmpc_simulate_device")).  bmpc_rollout_device closes the loop on the controller's own
 * prediction with feet that never move; these entries close it on a PLANT: the nonlinear single rigid body, with feet that land
 * where the swing controller steers them and an optional push.  What a rigid body makes of the controller, per instance.
 *
 * The plant.  State x = [e(3), p(3), w(3), v(3)], e = [roll, pitch, yaw], w and v in the world frame (REF:13).  Held over one control
 * period dt: the controls u = [f1 f2 m1 m2], the feet r_0, r_1, the contact bits c_0, c_1 and an external wrench [F(3), M(3)] in
 * the world frame.  With R = Rz(e2) Ry(e1) Rx(e0) (REF:124-138) and I_w = R I R':
 *   e0' = (cos e2 wx + sin e2 wy) / cos e1,  e1' = -sin e2 wx + cos e2 wy,  e2' = wz + sin e1 e0',  p' = v,
 *   w' = I_w^-1 (tau - w x I_w w),  tau = sum_g c_g [(r_g - p) x f_g + m_g] + M,   v' = (sum_g c_g f_g + F) / m + (0, 0, -g).
 * A leg whose contact bit is 0 transmits nothing.  This is not the controller's model (REF:148-185; DESIGN.md lists the
 * differences).  Integration: `substeps` in [1, 64] steps of dt / substeps, explicit Euler (BMPC_PLANT_EULER: every component from
 * the old stage values, the form of REF:183-184) or classical Runge-Kutta (BMPC_PLANT_RK4).  fp64 arithmetic on the fp32 arrays.
 * A non-finite input of an instance, or |cos e1| < 2^-22 at any stage, makes the whole next state of that instance NaN; no other
 * instance is touched.
 *   bmpc_plant_default(p)      RK4, 4 substeps, move_feet 1, no push
 *   bmpc_plant_step_device     one period: x_fb [B][12], u0 [B][12], foot [B][6], contact0 [B][2], wrench [B][6] or NULL
 *                              -> x_next [B][12].  DEVICE pointers, asynchronous on `stream`; move_feet / push_* are not used
 *   bmpc_plant_step            the same with HOST pointers, synchronous (staged through the handle's own stream)
 *
 * bmpc_simulate_device: bmpc_rollout_device's loop (schedule, optional longest-first order, solve; warm start and
 * bmpc_set_dispatch_order honoured alike; one stream, no host arithmetic, no synchronisation) with another feedback step.  Per
 * period s:  x_fb <- plant(x_fb, controls[:, 0], foot, row 0 of the period's contact table, push if push_from <= s < push_from +
 * push_steps);  t += dt;  with move_feet != 0, a leg whose row-0 contact bit is 0 at the old t and 1 at the new one (the gait rule of
 * bmpc_contact_sequence) LANDS: its foothold becomes the swing controller's target (REF:428-435) at the new state as stored (fp32),
 *   x = p_x + v_x (h / 2 dt) / 2 + kv (p_x - cmd_x),  y likewise + 0.04 side (side +1 for leg 0, -1 for leg 1),  z = 0,
 * with cmd the per-instance x_cmd where given, else the handle's; every other foothold stays.
 *   x_fb [B][12] in/out, foot [B][6] in/out, t [B] fp64 in/out; gait, x_cmd, mu as for bmpc_rollout_device; push [B][6] or NULL;
 *   u0_traj [steps][B][12], x_traj [steps][B][12] (state after each period), foot_traj [steps][B][6] (footholds after each period's
 *   update), iters_traj [steps][B], status_any [B] (OR of the per-period status values, and BMPC_NUMERICAL where a plant step went
 *   bad): each may be NULL.
 * `plant` NULL is the default.  substeps outside [1, 64], an unknown integrator, a negative push_from or push_steps (checked
 * first, before the handle), a NULL handle, or a NULL required pointer is BMPC_ERR_INVALID, before any device call; B == 0 (and
 * steps == 0) succeeds.
 */
enum bmpc_plant_integrator {
  BMPC_PLANT_EULER = 0,
  BMPC_PLANT_RK4 = 1
};
typedef struct bmpc_plant {
  int32_t integrator;        /* BMPC_PLANT_EULER / BMPC_PLANT_RK4 */
  int32_t substeps;          /* 1 .. 64 */
  int32_t move_feet;         /* bmpc_simulate_device: landing legs get a new foothold */
  int32_t push_from;         /* bmpc_simulate_device: first period of the push */
  int32_t push_steps;        /* ... and its number of periods (0: none) */
} bmpc_plant;
int bmpc_plant_default(bmpc_plant* p);
int bmpc_plant_step(bmpc_handle h, int B, const bmpc_plant* plant, const float* x_fb, const float* u0, const float* foot,
                    const uint8_t* contact0, const float* wrench, float* x_next);
int bmpc_plant_step_device(bmpc_handle h, int B, const bmpc_plant* plant, const float* x_fb, const float* u0, const float* foot,
                           const uint8_t* contact0, const float* wrench, float* x_next, void* stream);
int bmpc_simulate_device(bmpc_handle h, int B, int steps, const bmpc_plant* plant, float* x_fb, float* foot, double* t,
                         const bmpc_gait* gait, const float* x_cmd, const float* mu, const float* push,
                         float* u0_traj, float* x_traj, float* foot_traj,
                         int32_t* iters_traj, int32_t* status_any, void* stream);

/*
 * The plant with a body per instance, and the fall outcome of a simulation (added under ABI 13 like the entries above: detect
 * them by the symbol).  The entries above integrate the body the controller believes in: m, I, g of the handle's bmpc_params.
 * These take the PLANT's m, I and g per instance, so that one launch sequence answers what one controller model makes of
 * thousands of real bodies (a payload, a wrong inertia estimate, another gravity).  Everything that is the controller's stays the
 * handle's: the solve inside the loop reads the handle's parameter block as before, and kv, dt, h, the commands and the landing
 * rule are untouched.  There is no centre-of-mass offset (the lever arms still run from p), there are no per-instance controller
 * parameters, and an instance that has fallen keeps being solved and integrated.
 *   bmpc_plant_body   m [B], I [B][9] (row-major body inertia, any invertible matrix), g [B], fp64; a NULL member is the handle's
 *                     value.  I^-1 is formed per instance in fp64 (adjugate over determinant).  A bad body -- a non-finite value,
 *                     m <= 0, a determinant that is zero or non-finite, a non-finite entry of the inverse -- makes the next state of
 *                     that instance all NaN (in the closed loop: BMPC_NUMERICAL in status_any), like a bad state; no other instance
 *                     is touched.  `body` NULL, or all three members NULL: the entries above, bit for bit.
 *   bmpc_sim_outcome  per instance, reduced over the periods on the device.  An instance has FALLEN at period s iff
 *                     !(|x[0]| <= tilt_max && |x[1]| <= tilt_max && x[5] >= z_min) at the state stored after period s (fp32, widened
 *                     to fp64 for the comparison): a NaN state counts as fallen.  first_fall [B]: the smallest such s, or -1;
 *                     max_tilt [B]: the maximum over the periods of max(|x[0]|, |x[1]|); min_z [B]: the minimum of x[5]; both fp32,
 *                     over the periods whose value is not NaN, NaN if there is none.  The entry initialises the arrays on the
 *                     stream.  Each array may be NULL; `outcome` NULL or all three NULL: nothing is reduced.  A NaN threshold is
 *                     BMPC_ERR_INVALID (checked with the plant block, before the handle); +inf / -inf switch a threshold off.
 *   bmpc_plant_step_body_device / bmpc_plant_step_body   bmpc_plant_step_device / bmpc_plant_step with `body` (DEVICE / HOST
 *                     pointers, `body` members included)
 *   bmpc_simulate_body_device   bmpc_simulate_device with `body` (DEVICE pointers) and `outcome`; the same loop, another feedback step
 */
typedef struct bmpc_plant_body {      /* per-instance rigid body of the PLANT; each member NULL -> the handle's value */
  const double* m;                    /* [B]    */
  const double* I;                    /* [B][9] body inertia, row-major, any invertible matrix */
  const double* g;                    /* [B]    */
} bmpc_plant_body;
typedef struct bmpc_sim_outcome {
  double tilt_max, z_min;             /* NaN: BMPC_ERR_INVALID; +inf / -inf allowed */
  int32_t* first_fall;                /* [B] or NULL */
  float* max_tilt;                    /* [B] or NULL */
  float* min_z;                       /* [B] or NULL */
} bmpc_sim_outcome;
int bmpc_plant_step_body_device(bmpc_handle h, int B, const bmpc_plant* plant, const bmpc_plant_body* body, const float* x_fb,
                                const float* u0, const float* foot, const uint8_t* contact0, const float* wrench, float* x_next,
                                void* stream);
int bmpc_plant_step_body(bmpc_handle h, int B, const bmpc_plant* plant, const bmpc_plant_body* body, const float* x_fb,
                         const float* u0, const float* foot, const uint8_t* contact0, const float* wrench, float* x_next);
int bmpc_simulate_body_device(bmpc_handle h, int B, int steps, const bmpc_plant* plant, const bmpc_plant_body* body, float* x_fb,
                              float* foot, double* t, const bmpc_gait* gait, const float* x_cmd, const float* mu, const float* push,
                              float* u0_traj, float* x_traj, float* foot_traj, int32_t* iters_traj, int32_t* status_any,
                              const bmpc_sim_outcome* outcome, void* stream);

/*
 * A ground under the plant: friction cone, unilateral contact, and who slipped (added under ABI 13 like the entries above: detect
 * them by the symbol).  The entries above pass on whatever the controller asks for: a stance leg can pull on the ground and push
 * sideways with any force.  These put a flat floor with Coulomb friction between the controller and the body.  The rule is applied
 * per instance once per control period, before the integration, in fp64 on the fp32 controls (they are held over the period and the
 * ground is flat, so it does not depend on the state).  For leg g with contact bit c_g, commanded f = (fx, fy, fz), m and true
 * friction mu_g:
 *   c_g == 0                 the leg transmits nothing, as above: its 6 applied values are +0
 *   c_g == 1, not fz > 0     UNLOADED: the ground cannot pull and passes no moment without load; all 6 are +0; flag bit 4 << g
 *   c_g == 1, fz > 0         LOADED: with t = sqrt(fx fx + fy fy) and lim = mu_g fz, the leg SLIPS if t > lim: fx and fy are scaled
 *                            by lim / t in fp64, each rounded to fp32 once, flag bit 1 << g; otherwise fx and fy pass with their bits
 *                            (t == lim holds).  fz and m always pass with their bits.
 * mu_g may be +inf (no friction limit; it is multiplied for loaded legs only).  A mu_g that is NaN or negative, or a control that
 * is not finite (either leg, whatever its contact bit), is a bad instance: u_applied all NaN, flags 0, the next state all NaN,
 * BMPC_NUMERICAL in status_any, like a bad body; no other instance is touched.  The DEMAND of a period is the largest t / fz over the
 * loaded legs with fz >= fz_floor, NaN if there is none.  The plant integrates the applied controls as stored in fp32 with the same
 * contact bits: a ground step is exactly the body step at u_applied.
 * Limits: a slipping foot does not slide (its foothold stays); moments have no limit (no centre of pressure, no torsional
 * friction); static and kinetic friction are one number; the ground is flat at z = 0.
 *   bmpc_plant_ground   mu [B][2] per leg, fp64; NULL: the handle's params.mu for both legs -- the true cone against the
 *                       controller's pyramid.  The solve inside the loop keeps reading the handle's block and the caller's
 *                       mu [B][h][2], the controller's BELIEF, exactly as before.
 *   bmpc_ground_out     what the closed loop records of the ground; each pointer may be NULL.  The reduced arrays (first_slip,
 *                       slip_periods, unloaded_periods, mu_demand) are initialised by the entry on the stream (-1, 0, 0, NaN).
 *                       fz_floor NaN or negative is BMPC_ERR_INVALID (checked with the plant block, before the handle).
 *   bmpc_plant_step_ground_device / bmpc_plant_step_ground   bmpc_plant_step_body_device / bmpc_plant_step_body with `ground`
 *                       (DEVICE / HOST pointers, members and u_applied, flags included)
 *   bmpc_simulate_ground_device   bmpc_simulate_body_device with `ground` and `gout` (DEVICE pointers); u0_traj keeps recording the
 *                       controller's command
 * `ground` NULL runs the body entries, bit for bit; a non-NULL u_applied, flags or gout is then BMPC_ERR_INVALID (checked before
 * the handle).  `body` stays optional and `outcome` is reduced as before.
 */
typedef struct bmpc_plant_ground { const double* mu; } bmpc_plant_ground;   /* [B][2] per leg, fp64; NULL -> params.mu for both legs */
typedef struct bmpc_ground_out {
  double fz_floor;            /* mu_demand counts a leg only while fz >= fz_floor; >= 0; NaN or negative: BMPC_ERR_INVALID */
  float* u_applied;           /* [steps][B][12] what reached the body each period */
  uint8_t* flags;             /* [steps][B]: 1, 2 leg 0 / 1 slipped; 4, 8 leg 0 / 1 unloaded */
  int32_t* first_slip;        /* [B] first period with a slip bit, or -1 */
  int32_t* slip_periods;      /* [B][2] periods each leg slipped */
  int32_t* unloaded_periods;  /* [B][2] */
  float* mu_demand;           /* [B] max over the periods (fp32, NaN periods skipped), NaN if none */
} bmpc_ground_out;            /* each pointer may be NULL; the entry initialises the reduced arrays on the stream */
int bmpc_plant_step_ground_device(bmpc_handle h, int B, const bmpc_plant* plant, const bmpc_plant_body* body,
                                  const bmpc_plant_ground* ground, const float* x_fb, const float* u0, const float* foot,
                                  const uint8_t* contact0, const float* wrench, float* x_next, float* u_applied /* [B][12] or NULL */,
                                  uint8_t* flags /* [B] or NULL */, void* stream);
int bmpc_plant_step_ground(bmpc_handle h, int B, const bmpc_plant* plant, const bmpc_plant_body* body,
                           const bmpc_plant_ground* ground, const float* x_fb, const float* u0, const float* foot,
                           const uint8_t* contact0, const float* wrench, float* x_next, float* u_applied, uint8_t* flags);
int bmpc_simulate_ground_device(bmpc_handle h, int B, int steps, const bmpc_plant* plant, const bmpc_plant_body* body,
                                const bmpc_plant_ground* ground, float* x_fb, float* foot, double* t, const bmpc_gait* gait,
                                const float* x_cmd, const float* mu, const float* push, float* u0_traj, float* x_traj,
                                float* foot_traj, int32_t* iters_traj, int32_t* status_any, const bmpc_sim_outcome* outcome,
                                const bmpc_ground_out* gout, void* stream);

/*
 * S candidate plans per instance rolled out on the plant (added under ABI 13 like the entries above: detect them by the symbol).
 * bmpc_evaluate_samples* scores S whole plans per instance through the controller's linearised model; the plant entries above
 * integrate the rigid body for one control per instance and period.  These entries ask the rigid body what it makes of each of the
 * S whole plans: nonlinear predictive sampling / MPPI next to the QP solver, a check of a solver's plan against the body before it is
 * applied, and the model gap per plan (this cost minus bmpc_evaluate_samples' cost on the same reference).  One launch, one thread
 * per plan, nothing replicated; max_batch bounds B, not B S.  Inputs, for B instances:
 *   x_fb [B][12], foot [B][6], contact [B][h][2] (row k holds over period k), controls [B][S][h][12] fp32 (plan s of instance b);
 *   x_cmd [B][12] or NULL (the handle's), x_ref [B][h][12] or NULL (generated), push [B][6] or NULL;
 *   plant   integrator, substeps, move_feet, push_from, push_steps (NULL: the default);  body, ground  as above, each NULL as above
 *   price   S, the thresholds of the fall outcome, the floor of the demand, the prices of the score and the temperature (below)
 * Per period k = 0 .. h - 1 of plan (b, s):  u = controls[b][s][k];  with a ground, u_applied = what the ground transmits of u under
 * contact[b][k] and mu[b] (the rule above), else u_applied = u;  the wrench is push[b] while push_from <= k < push_from + push_steps;
 * the plant integrates the instance's body over the period and the new state is rounded to fp32 and STORED.  Period k + 1 starts
 * from the stored state and EVERY output refers to it, so a roll-out is exactly the chain of bmpc_plant_step_ground_device calls a
 * caller could make period by period.
 *   cost    sum_k sum_i Q_i (x_k,i - xr_k,i)^2 + R_i u_k,i^2, i = 0 .. 11, in fp64 in that order: x_k the state stored after period k,
 *           widened; u_k the COMMANDED control (as bmpc_evaluate* counts it, whatever the ground passed on); xr_k = x_ref[b][k] where
 *           supplied, else generated as the solve generates it (REF:61-70; row 0 is x_fb).  With generated references this cost and
 *           bmpc_evaluate_samples' cost are the same functional of two models.
 *   landing by the TABLE: with move_feet != 0 and k + 1 < h, leg g lands if contact[b][k][g] == 0 and contact[b][k + 1][g] == 1; its
 *           foothold becomes the swing controller's target (REF:428-435, the formula of bmpc_simulate_device) at the state stored
 *           after period k, rounded to fp32; every other foothold stays
 *   score   cost + w_fall [first_fall >= 0] + w_slip (slip_periods[0] + slip_periods[1])
 *                + w_unloaded (unloaded_periods[0] + unloaded_periods[1]), added in that order
 * Per-sample outputs, each optional: cost, score [B][S] fp64;  x_end [B][S][12], foot_end [B][S][6] (after the last landing),
 * x_traj [B][S][h][12] fp32;  first_fall [B][S] int32, max_tilt, min_z [B][S] fp32 (bmpc_sim_outcome's rules over the h periods);
 * first_slip [B][S], slip_periods [B][S][2], unloaded_periods [B][S][2] int32, mu_demand [B][S] fp32 (bmpc_ground_out's rules; they
 * need a ground).  Per-instance reductions, each optional: best, n_valid, weights, u_mean, ess exactly as in bmpc_samples_out, from
 * these scores and the commanded controls (the same kernel behind the first on the same stream; scores or weights the caller did
 * not ask for live in the handle's scratch, with the rules stated there).
 * A sample's values depend on nothing but its instance's inputs and its own controls: not on B, S, b or s.  A non-finite control
 * entry of sample s at period k, or a plant step that goes bad there (|cos pitch| < 2^-22 at a stage), makes that sample's state
 * NaN from period k on: its cost and score are NaN and its first_fall is k; no other sample is touched.  A bad INSTANCE makes every
 * sample of it so: a non-finite x_fb or foot entry, a bad body, a mu that is NaN or negative (period 0); a non-finite push (the
 * first period it acts in) or reference entry (the period of its row).
 * Not modelled, as for the ground: a slipping foot does not slide, moments have no limit, static and kinetic friction are one
 * number, the floor is flat at z = 0.  Bodies are per instance, not per sample; no noise is generated.
 *   bmpc_plant_rollout_samples_device   DEVICE pointers (members of body, ground and out included), asynchronous on `stream`
 *                                       (same rules as bmpc_evaluate_samples_device)
 *   bmpc_plant_rollout_samples          HOST pointers, synchronous (staged through the handle's own stream)
 * Checked before a device is touched, each BMPC_ERR_INVALID, in this order: `price` NULL, S outside [1, 65536], a price that is NaN,
 * negative or infinite, a temperature that is NaN or <= 0, a NaN threshold, fz_floor NaN or negative; the plant block as for
 * bmpc_simulate_device; first_slip, slip_periods, unloaded_periods or mu_demand wanted without a ground.  Then: a NULL handle, x_fb,
 * foot, contact, controls or `out`; all outputs NULL; B outside [0, max_batch].  B = 0 succeeds.
 * The handle's parameter block is read (bmpc_set_params takes effect) and none of its per-solve state is touched:
 * bmpc_last_kernel_ms keeps reporting the last SOLVE.
 */
typedef struct bmpc_rollout_price {
  int32_t S;                  /* samples per instance, 1 .. 65536 */
  int32_t reserved0;
  double  w_fall;             /* finite, >= 0: price of having fallen */
  double  w_slip;             /* ... of each period a leg slipped */
  double  w_unloaded;         /* ... of each period a stance leg was unloaded */
  double  temperature;        /* > 0, +inf allowed (uniform weights) */
  double  tilt_max, z_min;    /* fall thresholds as in bmpc_sim_outcome: not NaN; +inf / -inf switch one off */
  double  fz_floor;           /* as in bmpc_ground_out: >= 0, not NaN */
} bmpc_rollout_price;
typedef struct bmpc_rollout_out {     /* each NULL = not wanted; at least one non-NULL */
  double*  cost;              /* [B][S]        */
  double*  score;             /* [B][S]        */
  float*   x_end;             /* [B][S][12]    */
  float*   foot_end;          /* [B][S][6]     */
  float*   x_traj;            /* [B][S][h][12] */
  int32_t* first_fall;        /* [B][S]        */
  float*   max_tilt;          /* [B][S]        */
  float*   min_z;             /* [B][S]        */
  int32_t* first_slip;        /* [B][S]     (needs a ground, like the three below) */
  int32_t* slip_periods;      /* [B][S][2]     */
  int32_t* unloaded_periods;  /* [B][S][2]     */
  float*   mu_demand;         /* [B][S]        */
  int32_t* best;              /* [B]           */
  int32_t* n_valid;           /* [B]           */
  double*  weights;           /* [B][S]        */
  double*  u_mean;            /* [B][h][12]    */
  double*  ess;               /* [B]           */
} bmpc_rollout_out;
int bmpc_plant_rollout_samples_device(bmpc_handle h, int B, const float* x_fb, const float* foot, const uint8_t* contact,
                                      const float* x_cmd, const float* x_ref, const float* push, const float* controls,
                                      const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                                      const bmpc_rollout_price* price, const bmpc_rollout_out* out, void* stream);
int bmpc_plant_rollout_samples(bmpc_handle h, int B, const float* x_fb, const float* foot, const uint8_t* contact,
                               const float* x_cmd, const float* x_ref, const float* push, const float* controls,
                               const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                               const bmpc_rollout_price* price, const bmpc_rollout_out* out);

/*
 * Gradient of the plant roll-out (added under ABI 13 like the entries above: detect them by the symbol).  For plan (b, s) the
 * forward pass is exactly the roll-out of bmpc_plant_rollout_samples as stated above -- the period loop, the ground in front of the
 * step, the push window, the state rounded to fp32 and stored, landing by the contact table at the stored state, and
 *   cost = sum_k sum_i Q_i (x_k,i - xr_k,i)^2 + R_i u_k,i^2   on the stored states and the COMMANDED controls --
 * and the gradient is the discrete adjoint of that chain:
 *   rounding   the fp32 rounding of a stored state, and of a scaled tangential force in the ground rule, is taken as the identity
 *              in the derivative; the linearisation point is the stored (rounded) values
 *   period     x_k = Phi(x_k-1, ua_k, r_k; c_k, w_k) is the plant step, differentiated exactly: every substep, every RK4 stage, the
 *              rates through the three sincos, the plane rotations, I_b and I_b^-1, and the closed-form p, v updates
 *   ground     ua_k = T(u_k), differentiated on the branch the forward pass took: a swing leg or an unloaded stance leg has a zero
 *              Jacobian block, a loaded leg inside the cone the identity, a slipping leg the Jacobian of
 *              (fx, fy) mu fz / sqrt(fx^2 + fy^2) with respect to (fx, fy, fz); moments pass.  The R_i u^2 term always sees the command
 *   footholds  are part of the chain: Phi depends on r_k, and a leg that lands after period k takes the target, which is affine in
 *              x_k[3], x_k[9] and x_k[4], x_k[10].  A foothold costate (6 values) runs backwards, collects (dPhi/dr)' lambda each
 *              period, is folded into lambda_k at a landing through the target's coefficients with that leg's part zeroed, and what is
 *              left at k = 0 is grad_foot.  With move_feet == 0 nothing is folded
 *   held fixed (as bmpc_evaluate_grad does): the reference rows (generated rows depend on x_fb: that dependence is not
 *              differentiated), the commands, the body, mu, the push and the contact table.  The outcome and the slip counters are
 *              not differentiated and are not outputs here.
 * Outputs per plan, each optional, at least one wanted: cost [B][S] fp64; grad_u [B][S][h][12] fp64 = d cost / d controls;
 * grad_x0 [B][S][12] fp64 = d cost / d x_fb; grad_foot [B][S][6] fp64 = d cost / d foot; x_traj [B][S][h][12] fp32, the stored
 * states; first_bad [B][S] int32: -1, or the period from which the plan's state is NaN.  A plan that is bad by
 * bmpc_plant_rollout_samples' rules has cost and every gradient entry NaN; no other plan is touched.
 * Exactly: an entry of grad_u that the plant never sees -- a swing leg's six values in period k and, with a ground, an unloaded
 * stance leg's -- is the fp64 product 2.0 * R_i * (double)u, in that order; grad_u[h-1] depends on
 * lambda_h-1 = 2 Q (x_h-1 - xr_h-1) alone.
 *   bmpc_plant_rollout_grad_device   DEVICE pointers (members of body, ground and out included), asynchronous on `stream` unless the
 *                                    handle's scratch has to grow
 *   bmpc_plant_rollout_grad          HOST pointers, synchronous (staged through the handle's own stream)
 * One launch, one thread per plan.  The recorded states (where x_traj is not wanted), the footholds every period started with and
 * the substep states of the period being transposed live in scratch on the handle, allocated on demand:
 * B S (4 (12 h + 6 h) + 48 substeps) bytes at most; if it cannot be allocated the entry returns BMPC_ERR_ALLOC with nothing launched.
 * Checked before a device is touched, each BMPC_ERR_INVALID, in this order: S outside [1, 65536]; the plant block as for
 * bmpc_simulate_device; a NULL handle, x_fb, foot, contact, controls or `out`; all outputs NULL; B outside [0, max_batch].  B = 0
 * succeeds.  The handle's parameter block is read (bmpc_set_params takes effect) and none of its per-solve state is touched.
 */
typedef struct bmpc_rollout_grad_out {   /* each NULL = not wanted; at least one non-NULL */
  double*  cost;              /* [B][S]        */
  double*  grad_u;            /* [B][S][h][12] */
  double*  grad_x0;           /* [B][S][12]    */
  double*  grad_foot;         /* [B][S][6]     */
  float*   x_traj;            /* [B][S][h][12] */
  int32_t* first_bad;         /* [B][S]        */
} bmpc_rollout_grad_out;
int bmpc_plant_rollout_grad_device(bmpc_handle h, int B, int S, const float* x_fb, const float* foot, const uint8_t* contact,
                                   const float* x_cmd, const float* x_ref, const float* push, const float* controls,
                                   const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                                   const bmpc_rollout_grad_out* out, void* stream);
int bmpc_plant_rollout_grad(bmpc_handle h, int B, int S, const float* x_fb, const float* foot, const uint8_t* contact,
                            const float* x_cmd, const float* x_ref, const float* push, const float* controls,
                            const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                            const bmpc_rollout_grad_out* out);

/* Diagnostics: when device_buf (DEVICE pointer, [max_batch][16] int64) is non-NULL every later solve
 * writes per-instance shader-clock stamps {setup, block algebra, dense sweeps, total, iters,
 * factorisations, -, -, iteration phases P0..P5, stop test + adaptation, -}; NULL switches it off
 * (default).  Costs a few s_memtime per phase. */
int bmpc_debug_set_profile(bmpc_handle h, long long* device_buf);

/* Duration of the LAST bmpc_solve_batch* kernel launch made through this handle, measured with one pair of
 * HIP events recorded around the launch on the launch's stream (milliseconds); <0 if none.  Waits for
 * that launch.  A handle owns ONE event pair: with several launches in flight through the same handle
 * (back-to-back asynchronous calls, or calls on different streams) only the last one is reported, and it
 * is only meaningful if no other launch of this handle overlapped it. */
int bmpc_last_kernel_ms(bmpc_handle h, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* BMPC_H */
