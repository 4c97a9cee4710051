/*
 * rtpb.h -- C ABI of the MI355X-native sequential ray tracer (ray_trace_pb_amd).
 *
 * This is the drop-in boundary for the reference's hot path, QI2lab/ray_trace_pb @ 2024_10_08:
 *
 *   src/raytrace/raytrace.py:658-659  (System.ray_trace)
 *       for ii in range(len(self.surfaces)):
 *           rays = self.surfaces[ii].propagate(rays, materials[ii], materials[ii + 1])
 *
 * One rtpb_trace() call replaces that whole loop: every Surface.propagate of the system
 * (RefractingSurface RT:1160-1234, ReflectingSurface RT:1238-1303, PerfectLens RT:1601-1801 with
 * FlatSurface RT:1306-1347, PlaneMirror RT:1377-1412, SphericalSurface RT:1435-1535), every
 * propagate_ray2plane (RT:241-306) and every Material.n (materials.py:39-144) runs fused in one HIP
 * kernel per launch on gfx950 (Sellmeier / Constant n(lambda) evaluated in the kernel; other
 * materials looked up in (wavelength, n) tables the caller evaluated with the material's own code).  The history the reference builds with concatenate (RT:1229-1232) is
 * written plane by plane, straight to its final place in the caller's output buffer.
 *
 * Conventions
 *   - Plain C types only.  All ray buffers are caller-owned; the library never frees or retains them.
 *   - A ray is 8 values (x, y, z, dx, dy, dz, phase, wavelength) -- RT:1-13, RT:85-94.  Layout AOS
 *     stores a plane as [ray][8] (the reference's (P, N, 8) C order); layout SOA stores it as [8][ray].
 *   - History plane p: p = 0 is the input plane, p = 2i+1 the rays AT surface i, p = 2i+2 the rays
 *     AFTER surface i (RT:1229-1232, RT:1799).  `plane_mask` bit p selects which planes are stored;
 *     selected planes are packed in increasing p order into consecutive output slots.
 *   - Per-ray failures are not errors: they are NaN exactly as in the reference (miss RT:1506-1509,
 *     back-facing RT:1190-1192, TIR RT:1221, aperture RT:1225-1226/1293-1294, NA RT:1757-1760,
 *     backward RT:303-304/1401).
 *   - Every function returns RTPB_OK (0) or a negative RTPB_E_* code; rtpb_last_error() returns the
 *     message of the calling thread's last failure.  No C++ exception crosses the ABI.
 *   - Thread-safety: plans are immutable after creation and may be used from several threads at
 *     once; each (device, stream) pair must be driven by one thread at a time.
 */
#ifndef RTPB_H
#define RTPB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTPB_ABI_VERSION 10  /* 2: + *_tables generators, surface-hook kernels, sorted-table lookup
                                3: input element type separate from the storage type (in_dtype)
                                4: + rtpb_trace_checked (table-miss flag)
                                5: + rtpb_buffer_alloc / _free / _dlpack (placement-robust history buffers)
                                6: stream-ordered history buffers: rtpb_buffer_alloc takes the stream,
                                   + rtpb_buffer_record_stream / _held / _dlpack_discard
                                7: + rtpb_torch_alloc / rtpb_torch_free (torch MemPool segments),
                                   rtpb_buffer_stats; releasing a mapping synchronises the device;
                                   + rtpb_ray_fan_tables_wl / rtpb_collimated_rays_tables_wl (per-ray
                                   wavelengths)
                                8: + rtpb_trace_f64 / rtpb_trace_f32 (one-shot calls),
                                   rtpb_oneshot_plans / rtpb_oneshot_clear; freeing a library buffer
                                   never synchronises the device (retired mappings are released by the
                                   next allocation that maps new memory, or by rtpb_buffer_trim)
                                9: + rtpb_trace_packed (rtpb_trace_checked's arguments in one struct)
                                10: + rtpb_focus_stats / rtpb_focus_sweep (through-focus statistics);
                                    rtpb_spot_image / rtpb_image_sweep (spot images) and
                                    rtpb_wavefront_stats / rtpb_wavefront_sweep (wavefront statistics) and the
                                    four rtpb_*_sweep_collimated (collimated-beam sweeps) joined within 10, and
                                    so did rtpb_focus_sweep_variants / _variants_collimated (many systems in one
                                    fused pass), then rtpb_wavefront_sweep_variants / _variants_collimated and
                                    rtpb_final_rays_variants / _variants_collimated, then rtpb_footprint_stats /
                                    rtpb_footprint_sweep / rtpb_footprint_sweep_collimated (per-surface beam
                                    footprints and vignetting), then rtpb_spot_energy / rtpb_energy_sweep /
                                    rtpb_energy_sweep_collimated (encircled and ensquared energy), then
                                    rtpb_huygens_psf (the diffraction PSF of a plane), then rtpb_wavefront_map /
                                    rtpb_wavefront_map_sweep / rtpb_wavefront_map_sweep_collimated (pupil OPD
                                    maps), then rtpb_transmission_stats / rtpb_transmission_sweep /
                                    rtpb_transmission_sweep_collimated / rtpb_ray_transmission / rtpb_plan_media
                                    (Fresnel losses per surface and throughput), then rtpb_polarisation_stats /
                                    rtpb_polarisation_sweep / rtpb_polarisation_sweep_collimated /
                                    rtpb_ray_polarisation (two field vectors per ray through every surface) joined
                                    within 10: new symbols only, nothing existing changed */

/* ---- error codes ---------------------------------------------------------------------------- */
#define RTPB_OK 0
#define RTPB_E_INVALID (-1)   /* bad argument (kind, size, pointer, mask) */
#define RTPB_E_HIP (-2)       /* HIP runtime error */
#define RTPB_E_NODEV (-3)     /* no GPU / device index out of range */
#define RTPB_E_LIMIT (-4)     /* a compiled-in limit was exceeded (e.g. > RTPB_MAX_SURFACES) */

/* ---- enums ---------------------------------------------------------------------------------- */
/* surface kinds (reference classes) */
#define RTPB_FLAT 0          /* FlatSurface      RT:1306-1347 (refracting)          */
#define RTPB_SPHERE 1        /* SphericalSurface RT:1435-1535 (refracting)          */
#define RTPB_PLANE_MIRROR 2  /* PlaneMirror      RT:1377-1412 (reflecting)          */
#define RTPB_PERFECT_LENS 3  /* PerfectLens      RT:1558-1801 (ideal-lens mapping)  */

/* material kinds (Material.n overrides) */
#define RTPB_CONSTANT 0      /* Constant  MAT:59-79:  n = c[0]                                   */
#define RTPB_SELLMEIER 1     /* Material  MAT:39-51:  c = {b1,b2,b3,c1,c2,c3}; Vacuum = zeros    */
#define RTPB_POLY6 2         /* Ebaf11    MAT:128-144: c = {p0..p5}, n^2 = p0+p1 w^2+p2 w^-2+...
                                evaluated on the device with the device pow(): within 1 ulp of the
                                host's, but NumPy's SIMD power differs from libm pow on ~5 % of
                                inputs, so bit-exact callers lower Ebaf11 as RTPB_TABLE instead */
#define RTPB_TABLE 3         /* n looked up by exact wavelength match in a (wavelength, n) table
                                evaluated on the host by the material's own n() (user subclasses;
                                the Python front end also lowers Ebaf11 this way, see POLY6) */

/* data types and layouts */
#define RTPB_F64 0
#define RTPB_F32 1
#define RTPB_AOS 0
#define RTPB_SOA 1

/* surface-hook interaction modes (rtpb_interact) */
#define RTPB_REFRACT 0
#define RTPB_REFLECT 1

#define RTPB_MAX_SURFACES 63     /* history planes 0..2S must fit the 128-bit plane mask */
#define RTPB_MAX_TABLE (1 << 22) /* total (wavelength, n) entries over all TABLE materials */

/* ---- descriptors ---------------------------------------------------------------------------- */
typedef struct rtpb_surface {
    int32_t kind;           /* RTPB_FLAT ... */
    int32_t reserved;
    double center[3];       /* Surface.center (RT:1063) */
    double normal[3];       /* FlatSurface/PlaneMirror/PerfectLens .normal (RT:1320, 1389, 1576) */
    double input_axis[3];   /* Surface.input_axis (RT:1054): front-side test, sphere aperture axis */
    double radius;          /* SphericalSurface.radius (signed, RT:1445) */
    double radius_sq;       /* radius**2 exactly as the host evaluates it (RT:1499) */
    double aperture;        /* Surface.aperture_rad (RT:1069) */
    double focal_len;       /* PerfectLens.focal_len */
    double sin_alpha;       /* numpy.sin(PerfectLens.alpha) (RT:1758-1759) */
    double on_tol;          /* on-surface tolerance; 1e-12 reproduces RT:1343/1408/1528 */
} rtpb_surface;

typedef struct rtpb_material {
    int32_t kind;           /* RTPB_CONSTANT ... */
    int32_t table_len;      /* RTPB_TABLE: number of (wavelength, n) pairs */
    double c[6];            /* coefficients, see kinds */
    const double* table;    /* RTPB_TABLE: host pointer to table_len pairs {wavelength, n}, any order
                               (the library sorts them; lookups are binary searches); a NaN
                               wavelength key gives n(NaN).  Copied at plan creation. */
} rtpb_material;

typedef struct rtpb_plan rtpb_plan;   /* opaque: lowered system resident on the GPU(s) */

/* ---- library -------------------------------------------------------------------------------- */
int rtpb_abi_version(void);
const char* rtpb_last_error(void);
/* Number of visible GPUs (0 when none; never an error). */
int rtpb_device_count(void);
/* Release every device resource the library holds (plans must be destroyed first). */
int rtpb_shutdown(void);

/* ---- history buffers (ABI 5, stream-ordered since ABI 6) ---------------------------------------- */
/* Output buffers for large histories.  The 2S+1 planes of a history are written concurrently, and that
   write pattern runs 15-45 % slower into some physical placements -- physically contiguous memory in
   particular, which the first large allocations of a process on an unfragmented card often are -- while a
   plain fill of the same memory does not.  rtpb_buffer_alloc maps the buffer's physical
   memory in `chunk_bytes` chunks (0: 64 MiB) placed in the virtual range in a shuffled order (`seed`), so
   every buffer gets the fast rate.  The buffer is device memory like any other (pass `*ptr` to rtpb_trace).
   Streams -- PyTorch caching-allocator semantics, made explicit:
     * a buffer is allocated for `stream` (a hipStream_t, NULL = the device's null stream);
     * rtpb_buffer_record_stream(ptr, s) marks a use of the live buffer containing `ptr` on another stream
       `s` (returns 1, not an error, when `ptr` is not inside a live history buffer);
     * rtpb_buffer_free never blocks: it records an event on the allocation stream and on every recorded
       stream and keeps the buffer, still mapped, in a per-device pool;
     * the next rtpb_buffer_alloc of the same size on that device returns it and makes ITS stream wait for
       those events on the device (hipStreamWaitEvent): nothing the new owner queues can touch the memory
       before the previous owner's recorded uses have finished.
   The pool keeps the most recently freed buffer per device (rtpb_set_tuning("buffer_pool_buffers", k)
   keeps k, 0 none); an older one retires, still mapped.  Freeing and pooled allocations never block (ABI 8):
   retired buffers are unmapped and their physical memory released by the next allocation that maps new
   memory (after a device synchronisation; not while that allocation's stream is capturing a graph), by
   rtpb_buffer_trim and by rtpb_shutdown; their virtual ranges stay reserved, never reused.  rtpb_buffer_trim
   -- and rtpb_shutdown, and an allocation that finds the device full -- waits for the recorded uses and
   releases every pooled and retired buffer.  rtpb_buffer_held reports the bytes and buffers the pool still holds on `device`
   (-1: all devices).
   rtpb_buffer_dlpack wraps the whole buffer as a C-contiguous DLPack (v0.8 DLManagedTensor, device type
   ROCm) tensor of `ndim` extents `shape` and element type `dtype` (RTPB_F64 / RTPB_F32); ownership passes
   to the importer, whose call of the managed tensor's deleter frees the buffer.  rtpb_buffer_dlpack_discard
   runs that deleter for a managed tensor no importer consumed.  Replaces nothing in the reference (NumPy
   allocates its histories itself, RT:1229-1232). */
int rtpb_buffer_alloc(int32_t device, uint64_t bytes, uint64_t chunk_bytes, uint64_t seed, void* stream, void** ptr,
                      void** handle);
int rtpb_buffer_free(void* handle);
int rtpb_buffer_record_stream(const void* ptr, void* stream);
int rtpb_buffer_trim(void);
int rtpb_buffer_held(int32_t device, uint64_t* bytes, int32_t* buffers);
int rtpb_buffer_dlpack(void* handle, int32_t ndim, const int64_t* shape, int32_t dtype, void** managed);
int rtpb_buffer_dlpack_discard(void* managed);

/* ---- torch MemPool segments (ABI 7) ------------------------------------------------------------- */
/* The same shuffled-chunk memory as the segment allocator of PyTorch's caching allocator:
       torch.cuda.MemPool(torch.cuda.memory.CUDAPluggableAllocator("librtpb.so", "rtpb_torch_alloc",
                                                                    "rtpb_torch_free").allocator())
   (torch's alloc_fn / free_fn signatures: void* (size_t, int, hipStream_t), void (void*, size_t, int,
   hipStream_t)).  torch then caches, reuses stream-ordered (Tensor.record_stream), counts
   (torch.cuda.memory_allocated) and releases (empty_cache / out of memory) those segments itself; the library
   only maps a fresh buffer of `size` bytes (NULL on failure) and, on free, synchronises the device and unmaps
   it.  ray_trace_pb_amd's default device histories come from such a pool (_engine.history_pool).
   rtpb_buffer_stats fills up to n of: [0] live torch-pool segment bytes on `device` (-1: all), [1] their
   count, [2] reserved virtual bytes of released mappings (never reused), [3] their count,
   [4] buffers allocated with plain hipMalloc because [2] reached rtpb_set_tuning("buffer_dead_va_limit"),
   [5] torch segments allocated, [6] torch segments freed, [7] the dead-VA limit in bytes. */
void* rtpb_torch_alloc(int64_t size, int32_t device, void* stream);
void rtpb_torch_free(void* ptr, int64_t size, int32_t device, void* stream);
int rtpb_buffer_stats(int32_t device, uint64_t* out, int32_t n);

/* ---- plans: reference System + initial/final materials, lowered ----------------------------- */
/* Validates and stores the system.  `nmat` must equal `nsurf + 1` (RT:653-656: initial material,
   System.materials, final material).  `dtype` is the STORAGE type of the output history, RTPB_F64 or
   RTPB_F32; arithmetic is always float64 (the reference's numerics).  The input rays keep their own
   element type (`in_dtype` of the trace calls): float64 rays traced into an RTPB_F32 plan give the
   reference's float64 history rounded once to float32 (nothing is rounded before the arithmetic), and
   float32 rays are widened exactly, as NumPy promotes them in the reference. */
int rtpb_plan_create(const rtpb_surface* surfaces, int32_t nsurf,
                     const rtpb_material* materials, int32_t nmat,
                     int32_t dtype, rtpb_plan** plan_out);
int rtpb_plan_destroy(rtpb_plan* plan);

/* ---- tracing on device-resident buffers ----------------------------------------------------- */
/* Trace n_rays rays through the whole plan on `device`, asynchronously on `stream` (a hipStream_t,
   NULL = the device's null stream).
     rays_in          device pointer, n_rays rays in `in_layout` with elements of type `in_dtype`
                      (RTPB_F64 / RTPB_F32; SOA input must use the plan's dtype); SOA fields are
                      `in_field_stride` elements apart (>= n_rays).
     out              device pointer to slot 0 of the output; slots are `out_plane_stride` elements
                      apart (>= 8*n_rays); SOA fields are `out_field_stride` elements apart.
     plane_mask_lo/hi bits 0..63 / 64..127 select history planes 0..2S (see above).
   The output's element type is the plan's dtype. */
int rtpb_trace(const rtpb_plan* plan, int32_t device,
               const void* rays_in, int32_t in_dtype, int64_t n_rays, int32_t in_layout, int64_t in_field_stride,
               void* out, int32_t out_layout, int64_t out_plane_stride, int64_t out_field_stride,
               uint64_t plane_mask_lo, uint64_t plane_mask_hi, void* stream);
/* rtpb_trace plus a table-miss flag: `table_miss` (device pointer to one int32, may be NULL) is set to
   1 by the launch when some ray's wavelength is not a key of some RTPB_TABLE material of the plan (that
   ray's n would be NaN, unlike the material's own n()).  The caller zeroes it before the call and reads
   it after the stream has completed.  Lets a caller trace optimistically with the table keys of a
   previous bundle and re-trace with the bundle's own keys only on a miss (bit-identical either way). */
int rtpb_trace_checked(const rtpb_plan* plan, int32_t device,
                       const void* rays_in, int32_t in_dtype, int64_t n_rays, int32_t in_layout,
                       int64_t in_field_stride, void* out, int32_t out_layout, int64_t out_plane_stride,
                       int64_t out_field_stride, uint64_t plane_mask_lo, uint64_t plane_mask_hi, void* stream,
                       int32_t* table_miss);

/* rtpb_trace_checked with its arguments in one struct (same fields, same meaning; table_miss may be NULL).  For
   bindings whose per-argument marshalling costs more than the call (ctypes: ~0.2 us per argument): the caller keeps
   a filled struct per (plan, shape, planes, stream) and updates the buffer pointers between calls. */
typedef struct rtpb_trace_call {
    const rtpb_plan* plan;
    const void* rays_in;
    void* out;
    void* stream;
    int32_t* table_miss;
    int64_t n_rays;
    int64_t in_field_stride;
    int64_t out_plane_stride;
    int64_t out_field_stride;
    uint64_t plane_mask_lo;
    uint64_t plane_mask_hi;
    int32_t device;
    int32_t in_dtype;
    int32_t in_layout;
    int32_t out_layout;
} rtpb_trace_call;
int rtpb_trace_packed(const rtpb_trace_call* call);

/* ---- one-shot calls (the replacement of RT:658-659 without a plan handle) ------- */
/* The whole system in one call: `surfaces` (nsurf) and `materials` (nmat = nsurf + 1: initial material,
   System.materials, final material -- RT:653-656) as for rtpb_plan_create, device buffers as for rtpb_trace.
     rays_in  device pointer, n_rays x 8 AOS records of double (rtpb_trace_f64) / float (rtpb_trace_f32)
     out      device pointer: the history in the same element type (float: the float64 trace rounded once
              on store, float rays widened exactly -- as rtpb_trace with an RTPB_F32 plan)
     plane_mask_flags  0 = every plane 0..2S, (2S+1) x n_rays x 8 AOS: the reference's return value
              (RT:1229-1232); RTPB_PLANES_FINAL = plane 2S alone (n_rays x 8); RTPB_OUT_SOA = planes stored
              [8][n_rays] instead of [n_rays][8].  Other bits: RTPB_E_INVALID.  (Any other plane
              selection: rtpb_plan_create + rtpb_trace.)
   Asynchronous on `hip_stream` (NULL = the device's null stream).  The system is lowered into a plan once
   and cached by content (every descriptor byte and the (wavelength, n) pairs of RTPB_TABLE materials; the
   16 most recently used systems), so repeated calls with one system cost a compare of its descriptors.
   rtpb_oneshot_plans returns the number of cached plans; rtpb_oneshot_clear drops them (a plan still in
   use by a call on another thread is destroyed when that call returns; rtpb_shutdown clears them too). */
#define RTPB_PLANES_FINAL 0x1u
#define RTPB_OUT_SOA 0x2u
int rtpb_trace_f64(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials, int32_t nmat,
                   const double* rays_in, int64_t n_rays, double* out, uint32_t plane_mask_flags, int32_t device,
                   void* hip_stream);
int rtpb_trace_f32(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials, int32_t nmat,
                   const float* rays_in, int64_t n_rays, float* out, uint32_t plane_mask_flags, int32_t device,
                   void* hip_stream);
int rtpb_oneshot_plans(void);
void rtpb_oneshot_clear(void);

/* ---- tracing host buffers (NumPy in, NumPy out), sharded over several GPUs ------------------ */
/* rays_in: host, n_rays x 8 AOS of `in_dtype`.  out: host, nslots x n_rays x 8 AOS of the plan's dtype
   (nslots = popcount of the mask).
   Rays are split into contiguous index ranges, one per listed device (NULL/0 devices = device 0),
   each traced by its own host thread with chunked, double-buffered H2D / kernel / D2H copies.
   Synchronous: returns when `out` is complete. */
int rtpb_trace_host(const rtpb_plan* plan, const void* rays_in, int32_t in_dtype, int64_t n_rays, void* out,
                    uint64_t plane_mask_lo, uint64_t plane_mask_hi,
                    const int32_t* devices, int32_t n_devices);

/* ---- device ray generators (reference RT:45-161), written straight into device memory -------- */
/* get_ray_fan(pt, theta_max, n_thetas, wavelength, nphis, center_ray): ray k = iphi*n_thetas+itheta.
   These two evaluate cos/sin with the device libm (within 1 ulp of the host's); the *_tables variants
   below are bit-exact against the caller's NumPy. */
int rtpb_ray_fan(int32_t device, int32_t dtype, void* rays_out, const double pt[3], double theta_max,
                 int64_t n_thetas, int64_t nphis, const double center_ray[3], double wavelength,
                 void* stream);

/* get_collimated_rays(pt, displacement_max, n_disps, wavelength, nphis, phi_start, normal) (RT:99-161):
   ray k = idisp*nphis + iphi; `normal` must be a unit vector. */
int rtpb_collimated_rays(int32_t device, int32_t dtype, void* rays_out, const double pt[3], double displacement_max,
                         int64_t n_disps, int64_t nphis, double phi_start, const double normal[3], double wavelength,
                         void* stream);

/* Same two generators with every host-side constant supplied by the caller, so the device output is
   bit-identical to the caller's own NumPy evaluation of RT:45-161: ex/ey (or n1/n2) basis vectors,
   (cos, sin) pairs of the linspace thetas (2*n_thetas doubles) and of the phis (2*nphis doubles), and
   the offsets (n_disps doubles).  Tables are HOST pointers, copied before the call returns. */
int rtpb_ray_fan_tables(int32_t device, int32_t dtype, void* rays_out, const double pt[3], int64_t n_thetas,
                        int64_t nphis, const double center_ray[3], const double ex[3], const double ey[3],
                        const double* theta_cos_sin, const double* phi_cos_sin, double wavelength, void* stream);
int rtpb_collimated_rays_tables(int32_t device, int32_t dtype, void* rays_out, const double pt[3], int64_t n_disps,
                                int64_t nphis, const double normal[3], const double n1[3], const double n2[3],
                                const double* offsets, const double* phi_cos_sin, double wavelength, void* stream);
/* ABI 7: the same with one wavelength per ray -- the reference's "either floating point or an array the same
   size as n_disps * nphis" (RT:115; rays[:, 7] = wavelengths, RT:94 / RT:159).  `wavelengths` is a DEVICE
   pointer to n_thetas*nphis (n_disps*nphis) float64 values in ray-index order, 8-byte aligned, read by the
   kernel (stream-ordered); everything else as above. */
int rtpb_ray_fan_tables_wl(int32_t device, int32_t dtype, void* rays_out, const double pt[3], int64_t n_thetas,
                           int64_t nphis, const double center_ray[3], const double ex[3], const double ey[3],
                           const double* theta_cos_sin, const double* phi_cos_sin, const double* wavelengths,
                           void* stream);
int rtpb_collimated_rays_tables_wl(int32_t device, int32_t dtype, void* rays_out, const double pt[3],
                                   int64_t n_disps, int64_t nphis, const double normal[3], const double n1[3],
                                   const double n2[3], const double* offsets, const double* phi_cos_sin,
                                   const double* wavelengths, void* stream);

/* propagate_ray2plane(rays, normal, center, material, exclude_backward_propagation) (RT:241-306) on
   device rays (AOS n x 8).  normal / center: DEVICE pointers to 3 doubles (broadcast) or n x 3 doubles
   (*_per_ray = 1).  ts_out (device, n doubles) may be NULL.  workspace: device bytes for the material
   descriptor (>= 256 + 16 * max(table_len, 1)); the call synchronises `stream` after staging it.
   rays_in and rays_out must be 16-byte aligned (RTPB_E_INVALID otherwise).  A TABLE material's pairs may
   come in any order (the call sorts its copy); a SELLMEIER material with all-zero coefficients is Vacuum.
   n_rays == 0 returns RTPB_OK without reading the ray buffers, ts_out or the workspace (all may be NULL). */
int rtpb_propagate_plane(int32_t device, int32_t dtype, const void* rays_in, int64_t n_rays, const double* normal,
                         int32_t normal_per_ray, const double* center, int32_t center_per_ray,
                         const rtpb_material* material, int32_t exclude_backward, void* rays_out, double* ts_out,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* ---- user Surface subclasses with their own geometry (reference plugin point RT:1071-1156) ----- */
/* A Surface subclass that keeps RefractingSurface.propagate (RT:1160-1234) or
   ReflectingSurface.propagate (RT:1238-1303) but supplies its own get_intersect / get_normal /
   is_pt_on_surface.  The caller evaluates those three hooks; the library does the rest of propagate
   on the device.  `plan` holds ONE surface (only its input_axis is read) and TWO materials (the
   media before / after the surface); buffers are device pointers in the plan's storage type, rays
   AOS n x 8, normals n x 3.  The n x 8 buffers (rays, hits, hits_out, out) must be 16-byte aligned
   (RTPB_E_INVALID otherwise); normals and on_surface need only their element alignment.  n == 0 returns
   RTPB_OK without reading any buffer (all may be NULL).
   rtpb_front_side: hits_out = hits with every row NaN where rays.d . input_axis < 0 (RT:1184-1192);
     hits_out may equal hits.
   rtpb_interact: out = Snell refraction (mode RTPB_REFRACT, n1/n2 from the plan's materials at the
     hit's wavelength, RT:1194-1221) or reflection (RTPB_REFLECT, RT:1266-1289) of `hits` about
     `normals`, with position NaN where the direction is NaN (TIR) and the whole row NaN where
     on_surface[i] == 0 (RT:1225-1226; on_surface NULL = all on). */
int rtpb_front_side(const rtpb_plan* plan, int32_t device, const void* rays, const void* hits, int64_t n,
                    void* hits_out, void* stream);
int rtpb_interact(const rtpb_plan* plan, int32_t device, int32_t mode, const void* hits, const void* normals,
                  const uint8_t* on_surface, int64_t n, void* out, void* stream);

/* ---- device analysis ------------------------------------------------------------------------- */
/* intersect_rays(ray1, ray2) (RT:164-238) on device rays (AOS, n x 8; a length-1 side broadcasts).
   pts_out: max(n1, n2) x 3 intersection points, NaN where the rays do not meet within 1e-12. */
int rtpb_intersect_rays(int32_t device, int32_t dtype, const void* ray1, int64_t n1, const void* ray2, int64_t n2,
                        void* pts_out, void* stream);
/* Spot statistics of one (N, 8) AOS plane split into n_groups contiguous groups of group_size rays
   (e.g. one group per (field point, wavelength) fan).  Rays with non-finite x or y are skipped.
   stats_out (device, n_groups x 7 doubles): count, sum x, sum y, sum z, sum x^2, sum y^2, sum x*y.
   Deterministic (fixed-order two-pass reduction).  workspace: device doubles,
   >= n_groups * ceil(group_size / 256) * 7. */
int rtpb_spot_stats(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                    double* workspace, int64_t workspace_len, double* stats_out, void* stream);

/* Fused spot-diagram sweep (the C5 workload): for every group g the fan
   get_ray_fan(pt_g, theta_max, n_thetas, wavelength_g, nphis, center_ray) (RT:45-96) is generated,
   traced through `plan` (final state only) and reduced to the 7 statistics of rtpb_spot_stats -- one
   kernel, nothing but the statistics reaches HBM.  group_params: HOST, n_groups x {x, y, z, wavelength};
   ex/ey and the (cos, sin) tables as for rtpb_ray_fan_tables (host).  workspace: device doubles,
   >= n_groups * ceil(n_thetas*nphis / 256) * 7.  stats_out: device, n_groups x 7.  The statistics are
   bit-identical to rtpb_ray_fan_tables + rtpb_trace (final plane) + rtpb_spot_stats in the plan's
   storage type.  Groups with the same field point (bit for bit) are swept together -- each ray generated once
   and, when the first surface is a refracting flat or sphere, its wavelength-independent part computed once --
   so a call should hold all the wavelengths of its field points (order does not matter). */
int rtpb_spot_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                    int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                    const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin, double* workspace,
                    int64_t workspace_len, double* stats_out, void* stream);

/* Focus statistics of one (N, 8) AOS plane, per group as rtpb_spot_stats: the through-focus analysis of a
   bundle without tracing it again.  With the slopes u = dx / dz and v = dy / dz (IEEE division) a ray meets
   the plane displaced by delta along z at (x + u delta, y + v delta), so the RMS spot radius there is an
   exact quadratic in delta whose coefficients are second moments of (x, y, u, v).  A ray counts when x, y,
   u and v are all finite (dz = 0 and NaN or infinite directions drop it).
   stats_out (device, n_groups x 16 doubles): count, sum x, y, z, x^2, y^2, x*y (rtpb_spot_stats' columns, and
   its values bit for bit while every ray with finite x and y has finite slopes), then sum u, v, u^2, v^2,
   u*v, x*u, y*v, x*v, y*u.  The same fixed-order two-pass reduction.  workspace: device doubles,
   >= n_groups * ceil(group_size / 256) * 16.  The arguments are checked before the device is. */
int rtpb_focus_stats(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                     double* workspace, int64_t workspace_len, double* stats_out, void* stream);

/* Fused through-focus sweep: rtpb_spot_sweep with the 16 statistics of rtpb_focus_stats taken from each ray's
   final position and direction -- the same arguments, row planning and kernel.  workspace: device doubles,
   >= n_groups * ceil(n_thetas*nphis / 256) * 16.  stats_out: device, n_groups x 16.  The statistics are
   bit-identical to rtpb_ray_fan_tables + rtpb_trace (final plane) + rtpb_focus_stats in the plan's storage
   type.  The focus they describe lies along z: the last surface should be an image plane normal to z. */
int rtpb_focus_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                     int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                     const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin, double* workspace,
                     int64_t workspace_len, double* stats_out, void* stream);

/* Spot images: per group, a 2-D histogram of the final positions -- what a spot diagram shows when the rays are
   too many to scatter-plot or to store.  A group's window is four doubles {x_lo, y_lo, x_scale, y_scale}; the
   image has nx columns and ny rows, both at most RTPB_MAX_IMAGE_SIDE.  A ray COUNTS exactly when it counts for
   rtpb_spot_stats / rtpb_spot_sweep (x and y finite, in the storage type).  For a counting ray
   tx = (x - x_lo) * x_scale and ty = (y - y_lo) * y_scale (one rounded subtract, one rounded multiply); it is
   INSIDE iff 0 <= tx < nx and 0 <= ty < ny, compared in floating point, so NaN or infinite windows and
   overflowing products are outside; only then ix = (int)tx, iy = (int)ty and image[g][iy][ix] += 1.  A counting
   ray that is not inside adds 1 to outside[g]: image[g].sum() + outside[g] is the group's spot count, exactly.
   Integer counts: the result does not depend on the order in which rays arrive.
   image_out (device, n_groups*ny*nx int32) and outside_out (device, n_groups int32): each call zeroes its
   n_groups slices on `stream` before counting; no workspace.  At most 2^31 - 1 rays per group (RTPB_E_LIMIT).
   The arguments are checked before the device is.
   rtpb_spot_image: one (N, 8) AOS plane split into groups as for rtpb_spot_stats; windows: DEVICE, n_groups x 4. */
#define RTPB_MAX_IMAGE_SIDE 4096
int rtpb_spot_image(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                    const double* windows, int32_t nx, int32_t ny, int32_t* image_out, int32_t* outside_out,
                    void* stream);

/* Fused spot-image sweep: rtpb_spot_sweep with each counted ray binned into its group's image instead of summed --
   the same arguments, row planning and kernel, and its group and tile limits.  windows: HOST, n_groups x 4 (it
   rides in the sweep's one upload).  The images are identical to rtpb_ray_fan_tables + rtpb_trace (final plane)
   + rtpb_spot_image in the plan's storage type. */
int rtpb_image_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                     int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                     const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                     const double* windows, int32_t nx, int32_t ny, int32_t* image_out, int32_t* outside_out,
                     void* stream);

/* Wavefront statistics: per group, the moments of the optical path difference (OPD) from which the RMS wavefront
   error, the diffraction focus and the Marechal Strehl estimate follow on the host.  A group's REFERENCE is eight
   doubles {C0x, C0y, C0z, d0x, d0y, d0z, p0, kf}: the reference point C0, a pivot direction d0 and a pivot phase p0
   in radians (the group's chief ray), and kf = n_final(wavelength) / wavelength, evaluated by the caller.  The
   optical path of a ray to the foot of the perpendicular from C0 is linear in C0, so the variance of the OPD about
   C0 + delta is an exact quadratic in delta, and its coefficients are the moments summed here.  The pivots are
   subtracted per ray before anything is squared (un-pivoted sums of a 3e4 rad phase cancel to a few per cent).
   float64 ONLY: a float32 phase of 1e4 ... 1e7 rad has an ulp of a milliradian to a radian, so a float32 dtype or
   plan is RTPB_E_INVALID.  For a ray's final state (x, y, z, dx, dy, dz, ph), every operation one rounded IEEE
   operation in this order, no FMA:
       ex = dx - d0x;  ey = dy - d0y;  ez = dz - d0z
       s  = ((C0x - x) * dx + (C0y - y) * dy) + (C0z - z) * dz
       w  = (ph - p0) * 0.15915494309189535 + s * kf              (the OPD in waves; the constant is 1 / (2 pi))
   A ray COUNTS when rtpb_spot_stats counts it (x and y finite) and w, ex, ey and ez are all finite; a ray that does
   not count adds +0 to every sum.  A NaN in a group's reference makes every w NaN: the group counts 0.
   stats_out (device, n_groups x 15 doubles): count, sum w, w^2, ex, ey, ez, w*ex, w*ey, w*ez, ex^2, ey^2, ez^2,
   ex*ey, ex*ez, ey*ez, each product one rounded multiply; the fixed-order two-pass reduction of rtpb_spot_stats
   (a tree per 256-ray tile, then the tiles in a fixed order).  refs: HOST, n_groups x 8, uploaded on `stream`.
   workspace: device doubles, >= n_groups * ceil(group_size / 256) * 15.  The arguments are checked before the
   device is.
   rtpb_wavefront_stats: one (N, 8) AOS float64 plane split into groups as for rtpb_spot_stats. */
int rtpb_wavefront_stats(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                         const double* refs, double* workspace, int64_t workspace_len, double* stats_out,
                         void* stream);

/* Fused wavefront sweep: rtpb_focus_sweep's arguments with refs (HOST, n_groups x 8; it rides in the sweep's one
   upload) before the workspace, and its group and tile limits.  The surface steps are rtpb_trace's own (the phase
   is kept), every group is swept on its own, and the statistics are bit-identical to rtpb_ray_fan_tables +
   rtpb_trace (final plane) + rtpb_wavefront_stats.  workspace: device doubles,
   >= n_groups * ceil(n_thetas*nphis / 256) * 15.  stats_out: device, n_groups x 15.  float64 plans only. */
int rtpb_wavefront_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                         int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                         const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                         const double* refs, double* workspace, int64_t workspace_len, double* stats_out,
                         void* stream);

/* Fused sweeps of COLLIMATED BEAMS (objects at infinity): the four sweeps above with another source of rays.  For
   every group g the beam get_collimated_rays(pt_g, displacement_max, n_disps, wavelength_g, nphis, phi_start,
   normal_g) (RT:99-161) is generated, traced through `plan` (final state only) and reduced -- the same kernel with
   another generator, the same row planning, statistics, images and references, nothing but the results reaching HBM.
   group_params: HOST, n_groups x {x, y, z, wavelength}, the beam's point pt and its wavelength.
   group_frames: HOST, n_groups x 9 {normal, n1, n2}: the beam's direction (a unit vector) and the basis of its
   cross-section, n1 = (0,1,0) x normal (normal x (1,0,0) where that vanishes) and n2 = normal x n1, both normalised,
   evaluated by the caller as for rtpb_collimated_rays_tables.  offsets: HOST, n_disps doubles, the caller's
   linspace(-displacement_max, displacement_max, n_disps); phi_cos_sin: HOST, nphis (cos, sin) pairs of
   phi_start + 2 pi i / nphis.  Ray k = idisp * nphis + iphi of a group starts at
       pt + n1 * (off * cos phi) + n2 * (off * sin phi)        (each product and sum one rounded operation, no FMA)
   along normal with phase 0, every value rounded through the plan's storage type: the results are bit-identical to
   rtpb_collimated_rays_tables + rtpb_trace (final plane) + rtpb_spot_stats / rtpb_focus_stats / rtpb_spot_image /
   rtpb_wavefront_stats.  Groups with the same point AND the same frame (bit for bit) are swept together, as the
   fans of one field point are, so a call should hold all the wavelengths of its beams; beams that share a point and
   differ in direction are swept apart.  Workspace sizes (with n_disps*nphis rays per group), the 65535-group and
   tile limits, the float64-only rule of the wavefront call and the error codes are those of the fan calls; the
   arguments are checked before the device is. */
int rtpb_spot_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                               const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                               const double* phi_cos_sin, double* workspace, int64_t workspace_len,
                               double* stats_out, void* stream);
int rtpb_focus_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                                const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                                const double* phi_cos_sin, double* workspace, int64_t workspace_len,
                                double* stats_out, void* stream);
int rtpb_wavefront_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                    const double* group_params, const double* group_frames, int64_t n_disps,
                                    int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                    const double* refs, double* workspace, int64_t workspace_len, double* stats_out,
                                    void* stream);
int rtpb_image_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                                const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                                const double* phi_cos_sin, const double* windows, int32_t nx, int32_t ny,
                                int32_t* image_out, int32_t* outside_out, void* stream);

/* ENCIRCLED and ENSQUARED energy: per group, the fraction of the rays within radius r of a centre (EE50 / EE80 / EE90
   of a lens specification) and within a square of half-side r about it (detector pixels), as two histograms of nr
   equal bins over [0, r_max), 1 <= nr <= RTPB_MAX_ENERGY_BINS, and the distance of the farthest ray in each measure.
   A group's PARAMETERS are four doubles {cx, cy, scale, 0} with scale = nr / r_max, evaluated by the caller.  A ray
   COUNTS exactly when it counts for rtpb_spot_stats / rtpb_spot_image (x and y finite, in the storage type).  For a
   counting ray, every step one rounded IEEE operation in this order, no FMA:
       dx = x - cx;  dy = y - cy
       rho = sqrt(dx*dx + dy*dy)          (the correctly rounded square root)
       m   = max(|dx|, |dy|)
       tc  = rho * scale;   ts = m * scale
   The ray is INSIDE the circle curve iff 0 <= tc < nr, compared in floating point, so NaN or infinite parameters and
   overflowing products are outside; only then hist[g][0][(int)tc] += 1, otherwise outside[g][0] += 1.  The square
   curve is the same with ts, hist[g][1] and outside[g][1].  hist[g][k].sum() + outside[g][k] is the group's spot
   count, exactly, for both k.  farthest[g][0] is the largest rho over the counting rays and farthest[g][1] the
   largest m: 0.0 for a group with no counting ray, +inf where a product overflows; a NaN cannot arise from finite
   x, y and a finite centre.  A centre that is NOT FINITE (cx or cy NaN or infinite) puts every counting ray outside
   both curves and leaves farthest untouched (0.0 when all of the group's rays see it).  Integer counts and a
   maximum: the result does not depend on the order in which rays arrive (the maximum is an unsigned 64-bit atomic
   max on the bit pattern, non-negative doubles ordering as their bits).
   hist_out (device, n_groups*2*nr int32), outside_out (device, n_groups*2 int32), farthest_out (device, n_groups*2
   doubles): each call zeroes its n_groups slices on `stream` before counting; no workspace.  At most 2^31 - 1 rays
   per group (RTPB_E_LIMIT).  The arguments are checked before the device is.
   rtpb_spot_energy: one (N, 8) AOS plane split into groups as for rtpb_spot_stats; params: DEVICE, n_groups x 4. */
#define RTPB_MAX_ENERGY_BINS 4096
int rtpb_spot_energy(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                     const double* params, int32_t nr, int32_t* hist_out, int32_t* outside_out, double* farthest_out,
                     void* stream);

/* Fused energy sweeps: rtpb_image_sweep / rtpb_image_sweep_collimated with each counted ray added to its group's two
   curves instead of its image -- the same arguments up to the source's tables, row planning and kernel, and their
   group and tile limits.  params: HOST, n_groups x 4 (it rides in the sweep's one upload).  The results are
   identical to generating, tracing (final plane) and rtpb_spot_energy in the plan's storage type. */
int rtpb_energy_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                      int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                      const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                      const double* params, int32_t nr, int32_t* hist_out, int32_t* outside_out,
                      double* farthest_out, void* stream);
int rtpb_energy_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                                 const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                                 const double* phi_cos_sin, const double* params, int32_t nr, int32_t* hist_out,
                                 int32_t* outside_out, double* farthest_out, void* stream);

/* WAVEFRONT MAP: per group, the optical path difference over the exit pupil -- the interferogram, and what Zernike
   coefficients are fitted to on the host -- as a grid of nx x ny cells (each at most RTPB_MAX_IMAGE_SIDE) holding
   INTEGERS: how many rays fell into the cell and the sum of their OPDs in units of 2^-q_bits waves.  Integer adds do
   not depend on the order in which rays arrive, so the plane call, the fused sweeps and a host restatement agree bit
   for bit.  A group's REFERENCE is the wavefront calls' eight doubles {C0, d0, p0, kf}.  A group's WINDOW is four
   doubles {ex_lo, ey_lo, x_scale, y_scale} in the space of the direction offsets (ex, ey) = (dx - d0x, dy - d0y),
   with rtpb_spot_image's semantics exactly.  A ray COUNTS exactly when it counts for rtpb_wavefront_stats; w, ex and
   ey are that rule's values.  For a counting ray, every step one rounded IEEE operation in this order, no FMA:
       far_e = max(|ex|, |ey|);  far_w = |w|            (both enter farthest[g], whatever the window and w_lim say)
       tx = (ex - ex_lo) * x_scale;  ty = (ey - ey_lo) * y_scale
       INSIDE iff 0 <= tx < nx and 0 <= ty < ny (compared in floating point: a NaN or infinite window is outside);
           a ray that is not inside adds 1 to outside[g] and goes no further
       a ray that is inside and fails |w| <= w_lim adds 1 to clipped[g] (a failed comparison: a NaN never passes)
       otherwise tq = w * 2^q_bits (exact), q = (int64) rint(tq) (to nearest, ties to even), and with
           b = (int)ty * nx + (int)tx:  count[g][b] += 1 (int32),  sum[g][b] += q (int64)
   Two bounds follow: count[g].sum() + outside[g] + clipped[g] is the group's wavefront count n, exactly; and a cell's
   mean OPD sum / 2^q_bits / count is within 2^-(q_bits + 1) waves of the true mean of its rays.  farthest[g] =
   {max far_e, max far_w} over the counting rays (0.0 for a group with none; a NaN reference counts none): measured
   from the chief ray (e = 0), not from the window, so a call with any window -- a 1 x 1 map, say -- tells the caller
   which window and w_lim hold everything.  Unsigned 64-bit atomic maxima on the bit patterns, as rtpb_spot_energy's.
   The calls refuse what could overflow before a device is touched: RTPB_E_INVALID unless 0 <= q_bits <= 52 and w_lim
   is finite and >= 0; RTPB_E_LIMIT for more than 2^31 - 1 rays per group, and unless
       ldexp(w_lim, q_bits) + 1 <= ldexp(1.0, 62) / rays per group
   which keeps every cell's sum inside int64 by a factor of two (that covers the rounding of the check itself).
   count_out (device, n_groups*ny*nx int32), sum_out (device, n_groups*ny*nx int64), outside_out and clipped_out
   (device, n_groups int32), farthest_out (device, n_groups*2 doubles): each call zeroes its n_groups slices on
   `stream` before counting; no workspace.  float64 ONLY, for rtpb_wavefront_stats' reason.
   rtpb_wavefront_map: one (N, 8) AOS float64 plane split into groups as for rtpb_wavefront_stats; refs (n_groups x 8)
   and windows (n_groups x 4) are HOST pointers, uploaded by the call. */
int rtpb_wavefront_map(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                       const double* refs, const double* windows, int32_t nx, int32_t ny, int32_t q_bits,
                       double w_lim, int32_t* count_out, int64_t* sum_out, int32_t* outside_out, int32_t* clipped_out,
                       double* farthest_out, void* stream);

/* Fused wavefront map sweeps: rtpb_wavefront_sweep / rtpb_wavefront_sweep_collimated with each counted ray added to
   its group's map instead of the fifteen moments -- the same arguments up to the references, the same surface steps
   (the phase is the one rtpb_trace stores), float64 plans only, every group a single row; no workspace.  refs and
   windows: HOST (they ride in the sweep's one upload).  The results are identical to generating, tracing (final
   plane) and rtpb_wavefront_map. */
int rtpb_wavefront_map_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                             int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                             const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                             const double* refs, const double* windows, int32_t nx, int32_t ny, int32_t q_bits,
                             double w_lim, int32_t* count_out, int64_t* sum_out, int32_t* outside_out,
                             int32_t* clipped_out, double* farthest_out, void* stream);
int rtpb_wavefront_map_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                        const double* group_params, const double* group_frames, int64_t n_disps,
                                        int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                        const double* refs, const double* windows, int32_t nx, int32_t ny,
                                        int32_t q_bits, double w_lim, int32_t* count_out, int64_t* sum_out,
                                        int32_t* outside_out, int32_t* clipped_out, double* farthest_out,
                                        void* stream);

/* HUYGENS PSF: per group, the complex field on a grid of image-plane pixels as the coherent sum of the rays' plane
   wavelets -- the diffraction spot itself, from which the true Strehl ratio and the MTF follow on the host.  No
   interpolation, no triangulation, no FFT sampling constraint; a vignetted pupil is fewer rays.
   A group's REFERENCE is the wavefront calls' eight doubles {C0, d0, p0, kf}.  A group's WINDOW is four doubles
   {cx, cy, sx, sy}: pixel (ix, iy) of the nx x ny field lies at
       X = ((double)ix - cx) * sx;   Y = ((double)iy - cy) * sy        (one rounded subtract, one rounded multiply)
   from C0 in the image plane, so with cx = (nx - 1) / 2 the centre pixel is exactly C0.  float64 ONLY, for the
   wavefront calls' reason (a float32 dtype is RTPB_E_INVALID).  Per ray j of a group, with (n, w, ex, ey) the count
   flag, the OPD in waves and the direction offset that the wavefront statistics define above (the same operations,
   the same counting rule), every step one rounded IEEE operation in this order, no FMA:
       a  = n * weight[j]                      (weight[j] = 1 when weights == NULL)
       qx = ex * kf;   qy = ey * kf
   and per (ray, pixel):
       t  = (w + qx * X) + qy * Y
       fr = t - rint(t)                        (exact; |fr| <= 0.5: whole waves leave before the sine is taken)
       (s, c) = sincospi(2 * fr)               (the device library's double sincospi)
       re += a * c;   im += a * s
   e = d - d0 in d's place removes a linear phase common to all rays: |E|^2 is unchanged and t stays small.
   A ray that does NOT COUNT adds nothing: it is skipped, not multiplied by zero, so a NaN weight on a dead ray, or
   a NaN window, cannot reach the sum through it.  On a counting ray a non-finite t or a propagates: a NaN or
   infinite window entry, or a NaN weight on a live ray, gives NaN in every pixel it touches (a NaN window: the
   group's whole field).  A NaN in the reference makes every ray not count: the field is +0 everywhere and the norm
   0, whatever the window.
   field_out (device, n_groups * ny * nx * 2 doubles): re, im interleaved, pixel (ix, iy) of group g at
   ((g * ny + iy) * nx + ix) * 2: it views as complex128 (n_groups, ny, nx).  norm_out (device, n_groups doubles): the
   sum of a over the group's counting rays, the amplitude an aberration-free wavefront reaches at C0, so
   |E|^2 / norm^2 at C0 is the Strehl ratio.  Every element of both is written: the caller need not clear them.
   DETERMINISTIC: each pixel's sums, and the norm, are taken in an order fixed by (group_size, nx, ny) alone: the
   rays are split into segments of whole 256-ray tiles (as many as spread a group over about 1024 blocks, one where
   the window alone does), one thread adds a segment's rays in ray order, and a second pass adds the segments'
   partial sums in segment order.  No atomics; two calls give the same bits, whatever the stream and however the
   groups are divided among calls.
   plane: one (N, 8) AOS float64 plane split into groups as for rtpb_wavefront_stats.  refs: HOST, n_groups x 8;
   windows: HOST, n_groups x 4 (one upload on `stream`); weights: DEVICE, group_size doubles shared by all groups, or
   NULL.  1 <= nx, ny <= RTPB_MAX_PSF_SIDE (RTPB_E_LIMIT above, RTPB_E_INVALID below), n_groups <= 65535
   (RTPB_E_LIMIT), group_size >= 1; no workspace (the partial sums of split groups are stream-ordered scratch of at
   most 256 MiB).  The cost is group_size * nx * ny sincospi per group.  The
   arguments are checked before the device is. */
#define RTPB_MAX_PSF_SIDE 2048
int rtpb_huygens_psf(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                     const double* refs, const double* windows, const double* weights, int32_t nx, int32_t ny,
                     double* field_out, double* norm_out, void* stream);

/* FOOTPRINT statistics: per (group, surface), how many rays reach the surface, how many it lets through, and how much
   of it the beam uses -- which surface vignettes which field, and the clear semi-diameter each surface needs.  They
   are defined on the history rtpb_trace stores with every plane: for surface s and one ray, A is the ray's row in
   plane 2s + 1 (at the surface: the intersection point, kept where it lies outside the aperture) and B its row in
   plane 2s + 2 (after it).  A surface's FRAME is nine doubles {o, e1, e2}: an origin and two unit vectors spanning the
   plane the footprint is measured in, chosen by the caller.  float64 ONLY (a float32 dtype or plan is
   RTPB_E_INVALID).  Every operation one rounded IEEE operation in this order, no FMA:
       the ray ARRIVES when A.x, A.y, A.z are all finite; it PASSES when it arrives and B.x, B.y, B.z are all finite
       q = A.xyz - o;   u = (q.x*e1.x + q.y*e1.y) + q.z*e1.z;   v likewise with e2;   rho2 = u*u + v*v
   stats_out (device, n_groups x nsurf x 8 doubles), per (group, surface):
       0  the number of rays that arrive           1  the number of rays that pass
       2  max rho2 over the arriving rays (the aperture that would pass all that reaches the surface)
       3  max rho2 over the passing rays (the aperture in use)
       4, 5  min and max of u over the passing rays        6, 7  min and max of v over the passing rays
   An empty set gives -inf for a maximum and +inf for a minimum; a NaN u, v or rho2 (overflow only) is skipped by the
   comparisons (fmax / fmin) and the ray still counts.  Counts, maxima and minima only: the result does not depend on
   the order of the rays, so the two-pass reduction (a partial per block, then a group's blocks) is exact.
   frames: HOST, nsurf x 9, every entry finite, uploaded on `stream`.  nsurf <= RTPB_MAX_SURFACES, n_groups <= 65535
   (RTPB_E_LIMIT beyond).  The arguments are checked before the device is.
   rtpb_footprint_stats: a stored float64 AOS history [1 + 2 nsurf][n_groups * group_size][8], planes contiguous (what
   rtpb_trace writes with every plane selected), the rays of group g at rows g * group_size ... of each plane.
   workspace: device doubles, >= n_groups * ceil(group_size / 256) * nsurf * 8. */
int rtpb_footprint_stats(int32_t device, int32_t dtype, const void* history, int64_t group_size, int64_t n_groups,
                         int32_t nsurf, const double* frames, double* workspace, int64_t workspace_len,
                         double* stats_out, void* stream);

/* Fused footprint sweep: rtpb_wavefront_sweep's arguments with frames (HOST, n_frames x 9; it rides in the sweep's one
   upload) and n_frames, which must be the plan's number of surfaces, in the references' place.  The surface steps are
   those of rtpb_trace with every plane stored (the at-plane is formed, total internal reflection fills the position),
   run once per ray; no plane reaches HBM, so the sweep runs where no history fits.  Every group is swept on its own.
   CONTRACT: stats_out (device, n_groups x nsurf x 8) is bit-identical to rtpb_footprint_stats of the stored history of
   the same rays (rtpb_ray_fan_tables / rtpb_collimated_rays_tables + rtpb_trace, every plane) with the same frames.
   workspace: device doubles, >= n_groups * ceil(ceil(rays per group / 256) / 2) * nsurf * 8 (one partial per block of
   two tiles).  float64 plans only; the group and tile limits and error codes of rtpb_wavefront_sweep. */
int rtpb_footprint_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                         int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                         const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                         const double* frames, int32_t n_frames, double* workspace, int64_t workspace_len,
                         double* stats_out, void* stream);
int rtpb_footprint_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                    const double* group_params, const double* group_frames, int64_t n_disps,
                                    int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                    const double* frames, int32_t n_frames, double* workspace, int64_t workspace_len,
                                    double* stats_out, void* stream);

/* TRANSMISSION statistics: per (group, surface), how much LIGHT gets through -- Fresnel's equations for uncoated
   refracting surfaces at each ray's own angle of incidence, or a constant per surface: the loss per surface, the
   throughput per group and the apodisation across the pupil.  Defined on the stored history, like the footprints: for
   surface s and one ray, A is the ray's row in plane 2s + 1 (the position at the surface and the INCOMING direction),
   B its row in plane 2s + 2 (the OUTGOING direction), n1 and n2 the indices before and after the surface at the
   group's wavelength.  float64 ONLY (a float32 dtype or plan is RTPB_E_INVALID).  Every operation one rounded IEEE
   operation in this order, no FMA:
       the ray PASSES surface s exactly when the footprint statistics say so: A.xyz finite and B.xyz finite
       a surface's COATING is two doubles {mode, value}:
         mode 0, CONSTANT: t = value, 0 <= value <= 1 (an ideal lens, a mirror's reflectance, an AR coating as a number)
         mode 1, FRESNEL (uncoated, unpolarised; value is ignored): t = 1 where n1 == n2; else, dA = A.dxyz, dB = B.dxyz,
           g  = n1*dA - n2*dB                      (componentwise; by Snell's law g is along the normal)
           p1 = |(dA.x*g.x + dA.y*g.y) + dA.z*g.z|      p2 = |(dB.x*g.x + dB.y*g.y) + dB.z*g.z|
           rs = (n1*p1 - n2*p2) / (n1*p1 + n2*p2)       rp = (n2*p1 - n1*p2) / (n2*p1 + n1*p2)
           t  = 1 - 0.5*(rs*rs + rp*rp);   a t that is NaN or outside [0, 1] becomes 0
       cum_s = cum_(s-1) * t_s in surface order, cum_(-1) = 1 (a ray that passes s has passed every earlier surface)
       qt = rint(t * 2^q_bits),   qc = rint(cum * 2^q_bits)
   The rule uses no normal, no surface kind, no square root and no normalisation (|g| cancels in both ratios), so it
   holds for every surface that refracts by Snell's law.  What it is NOT: no polarisation state is carried from surface
   to surface (each surface sees unpolarised light), there is no absorption, and there are no thin-film stacks.
   stats_out (device, n_groups x nsurf x 5 doubles, all integer-valued or infinite), per (group, surface):
       0  the number of rays that pass        1  the sum of qt over them        2  the sum of qc over them
       3  min qc over them (+inf for none)    4  max qc over them (-inf for none)
   1 <= q_bits <= 40 (RTPB_E_INVALID otherwise); rays per group * 2^q_bits <= 2^53 (RTPB_E_LIMIT beyond): every sum is
   then an exact integer in a double in any order, so the two-pass reduction, any batching and any split over devices
   give the same bits.
   media: HOST, n_groups x (nsurf + 1) indices (rtpb_plan_media).  coatings: HOST, nsurf x 2, every entry finite, mode 0
   or 1, value in [0, 1] (RTPB_E_INVALID otherwise); both are uploaded on `stream`.  nsurf <= RTPB_MAX_SURFACES,
   n_groups <= 65535 (RTPB_E_LIMIT beyond).  The arguments are checked before the device is.
   rtpb_transmission_stats: a stored float64 AOS history as rtpb_footprint_stats takes it.
   workspace: device doubles, >= n_groups * ceil(group_size / 256) * nsurf * 5. */
int rtpb_transmission_stats(int32_t device, int32_t dtype, const void* history, int64_t group_size, int64_t n_groups,
                            int32_t nsurf, const double* media, const double* coatings, int32_t q_bits,
                            double* workspace, int64_t workspace_len, double* stats_out, void* stream);

/* Each ray's energy weight, for a caller's own apodised sums: out (device, one double per ray of the history) holds cum
   after the last surface, unquantised, NaN for a ray that does not pass it.  The arguments and checks of
   rtpb_transmission_stats without q_bits and the workspace. */
int rtpb_ray_transmission(int32_t device, int32_t dtype, const void* history, int64_t group_size, int64_t n_groups,
                          int32_t nsurf, const double* media, const double* coatings, double* out, void* stream);

/* The indices a float64 sweep of `plan` traces with: out (HOST, n x (nsurf + 1)) holds n of every material of the plan
   at wavelengths[i] (HOST, n of them), by the host arithmetic that fills the fused sweeps' media table.  Host only: no
   device is touched.  A float32 plan is RTPB_E_INVALID.  A plan with an RTPB_POLY6 material is RTPB_E_INVALID as well:
   that polynomial is evaluated on the device with the device's pow(), which the host does not reproduce bit for bit --
   lower the material as RTPB_TABLE at the call's wavelengths instead (the variant sweeps' rule).  The fused
   transmission sweeps refuse the same plans with the same code. */
int rtpb_plan_media(const rtpb_plan* plan, const double* wavelengths, int64_t n, double* out);

/* Fused transmission sweep: rtpb_footprint_sweep's arguments with coatings (HOST, n_coatings x 2; they ride in the
   sweep's one upload), n_coatings, which must be the plan's number of surfaces, and q_bits in the frames' place.  The
   surface steps are the footprint sweep's; the rule reads the indices the kernel traces with, so nothing is uploaded
   per group.
   CONTRACT: stats_out (device, n_groups x nsurf x 5) is bit-identical to rtpb_transmission_stats of the stored history
   of the same rays with the media rtpb_plan_media gives for the groups' wavelengths.
   workspace: device doubles, >= n_groups * ceil(ceil(rays per group / 256) / 2) * nsurf * 5.  float64 plans without
   POLY6 media only; the group and tile limits and error codes of rtpb_footprint_sweep. */
int rtpb_transmission_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                            int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                            const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                            const double* coatings, int32_t n_coatings, int32_t q_bits, double* workspace,
                            int64_t workspace_len, double* stats_out, void* stream);
int rtpb_transmission_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                       const double* group_params, const double* group_frames, int64_t n_disps,
                                       int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                       const double* coatings, int32_t n_coatings, int32_t q_bits, double* workspace,
                                       int64_t workspace_len, double* stats_out, void* stream);

/* POLARISATION statistics: two real field vectors per ray carried through every surface -- what the transmission
   statistics leave out.  Each ray is launched behind a linear polariser along the unit vector `polariser` with the
   STATE E1 (the axis projected across the ray, unit length) and E2 = ray x E1, or with NO state (all NaN); |E|^2 is
   energy.  Defined on the stored history like the transmission statistics, with their A, B, n1, n2 and media; a = A.dxyz
   and b = B.dxyz are the incoming and outgoing directions.  float64 ONLY.  Every operation one rounded IEEE operation
   in this order, no FMA, with p.q = (p.x*q.x + p.y*q.y) + p.z*q.z, p x q = (p.y*q.z - p.z*q.y, p.z*q.x - p.x*q.z,
   p.x*q.y - p.y*q.x) and sqrt correctly rounded:
       LAUNCH from the ray's first direction a (plane 0), u = polariser:
         c = a x u, cc = c.c; !(cc >= 2^-40): no state.  Else w = c x a, E1 = w / sqrt(w.w), E2 = a x E1
       the ray PASSES surface s exactly when the transmission statistics say so; a ray that does not has no state
       from then on
       a surface's COATING is two doubles {mode, value}, value in [0, 1]; amplitude = sqrt(value), formed once per call:
         mode 0, CONSTANT: ts = tp = amplitude.   mode 1, FRESNEL (value ignored): ts = tp = 1 where n1 == n2; else
           ts = sqrt(1 - rs*rs), tp = sqrt(1 - rp*rp) with the transmission rule's rs and rp (flux-normalised
           amplitudes: no n*cos factor appears).  Then c = a x b, cc = c.c, d = 1 + a.b; !(d >= 2^-20): no state; else
           for E = E1 and E = E2:
             k  = (ts - tp)*((E.c)/cc) where cc >= 2^-900, else 0
             E' = tp*E + k*c                     f = (E'.b)/d                     E_out = E' - (a + b)*f
           (the s and p amplitudes about the plane of incidence, then the minimal rotation that takes a to b:
           E_out.b = 0 by construction)
         mode 2, MIRROR (value: the reflectance): m = a - b, mm = m.m; !(mm >= 2^-40): no state; else
             g = (E.m)/mm                        E_out = amplitude*((2*g)*m - E)
       the ANALYSER after the surface, w = analyser (a unit vector): x = b x w, xx = x.x; p = E_i.x, l_i = (p*p)/xx:
       the energy of state i behind an analyser CROSSED with w
       the ray is VALID at s when it passes, all six components of E_out are finite and xx >= 2^-40
       q(v) = rint((v <= 1 ? v : 1) * 2^q_bits)
   What it is NOT: the amplitudes are real -- no retardance (total internal reflection, metal mirrors), no thin films,
   no birefringence; the state of a ray that totally reflects at a refracting surface ends.
   stats_out (device, n_groups x nsurf x 6 doubles, all integer-valued), per (group, surface):
       0  the rays that pass      1  the valid rays      2, 3  the sums of q(E1.E1) and q(E2.E2) over the valid rays
       4, 5  the sums of q(l1) and q(l2) over them
   q_bits, media, coatings, the limits and the order of the checks are rtpb_transmission_stats's, with mode 2 allowed;
   polariser and analyser: HOST, three doubles each, finite and not all zero (RTPB_E_INVALID otherwise), taken as
   given -- the caller normalises them.
   workspace: device doubles, >= n_groups * ceil(group_size / 256) * nsurf * 6. */
int rtpb_polarisation_stats(int32_t device, int32_t dtype, const void* history, int64_t group_size, int64_t n_groups,
                            int32_t nsurf, const double* media, const double* coatings, const double polariser[3],
                            const double analyser[3], int32_t q_bits, double* workspace, int64_t workspace_len,
                            double* stats_out, void* stream);

/* Each ray's two final field vectors, for a caller's own sums (a vectorial PSF, say): out (device, 6 doubles per ray of
   the history: E1.xyz, E2.xyz) holds the state after the last surface, unquantised, NaN for a ray without one.  The
   arguments and checks of rtpb_polarisation_stats without the analyser, q_bits and the workspace. */
int rtpb_ray_polarisation(int32_t device, int32_t dtype, const void* history, int64_t group_size, int64_t n_groups,
                          int32_t nsurf, const double* media, const double* coatings, const double polariser[3],
                          double* out, void* stream);

/* Fused polarisation sweep: rtpb_transmission_sweep's arguments with the two axes between n_coatings and q_bits.  The
   surface steps are the footprint sweep's; the state is launched from the generated ray's direction and carried in
   registers.
   CONTRACT: stats_out (device, n_groups x nsurf x 6) is bit-identical to rtpb_polarisation_stats of the stored history
   of the same rays with the media rtpb_plan_media gives for the groups' wavelengths.
   workspace: device doubles, >= n_groups * ceil(ceil(rays per group / 256) / 2) * nsurf * 6.  float64 plans without
   POLY6 media only; the group and tile limits and error codes of rtpb_transmission_sweep. */
int rtpb_polarisation_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                            int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                            const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                            const double* coatings, int32_t n_coatings, const double polariser[3],
                            const double analyser[3], int32_t q_bits, double* workspace, int64_t workspace_len,
                            double* stats_out, void* stream);
int rtpb_polarisation_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                       const double* group_params, const double* group_frames, int64_t n_disps,
                                       int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                       const double* coatings, int32_t n_coatings, const double polariser[3],
                                       const double analyser[3], int32_t q_bits, double* workspace,
                                       int64_t workspace_len, double* stats_out, void* stream);

/* VARIANT sweeps (tolerance runs): rtpb_focus_sweep / rtpb_focus_sweep_collimated over MANY systems in one call.
   The systems come in the call, as in rtpb_trace_f64: there is no plan and no per-system device memory.
   surfaces: HOST, n_variants x nsurf descriptors, variant v's at surfaces + v * nsurf; materials: HOST, n_variants x
   (nsurf + 1), variant v's at materials + v * (nsurf + 1) (initial medium, the media between the surfaces, final
   medium).  Every variant has the same number of surfaces; their kinds, geometry and media may all differ.
   dtype: the storage type (RTPB_F64 / RTPB_F32), a plan's dtype.  group_variant: HOST, n_groups, the variant in
   [0, n_variants) group g is traced through.  The remaining arguments are those of rtpb_focus_sweep from n_thetas on
   (rtpb_focus_sweep_collimated from group_frames on), and stats_out (DEVICE, n_groups x 16) holds the same sums.
   CONTRACT: the statistics of a group of variant v are bit-identical to those rtpb_focus_sweep[_collimated] gives
   the same group on a plan created (rtpb_plan_create) from variant v's descriptors with storage type dtype --
   whatever other variants and groups the call holds.  Groups are swept together when they share the source of their
   rays (the point; for beams the frame too) AND the variant, so a call should hold all the wavelengths of a field.
   Each variant is checked and lowered on the host by rtpb_plan_create's own code, and its descriptors ride in the
   call's one upload.  Media are evaluated on the host: a RTPB_POLY6 material (whose device arithmetic the host does
   not reproduce) is RTPB_E_INVALID -- lower it as RTPB_TABLE at the call's wavelengths.
   Everything is checked before the device is touched.  RTPB_E_INVALID: a NULL pointer, a non-positive nsurf,
   n_variants, n_groups or table size, a short workspace (n_groups * ceil(rays per group / 256) * 16 doubles), a
   group_variant entry outside [0, n_variants), a bad descriptor, a POLY6 material.  RTPB_E_LIMIT: nsurf >
   RTPB_MAX_SURFACES, n_groups > 65535, or an upload beyond RTPB_MAX_VARIANT_UPLOAD bytes, counted as
       16 (n_thetas + nphis) + n_groups (8 (4 nsurf + 5) + 12) + 280 n_variants nsurf
   (a collimated call: 72 n_groups more) -- split such a run into several calls. */
#define RTPB_MAX_VARIANT_UPLOAD (256ll << 20)
int rtpb_focus_sweep_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                              int32_t n_variants, int32_t dtype, int32_t device, int64_t n_groups,
                              const double* group_params, const int32_t* group_variant, int64_t n_thetas,
                              int64_t nphis, const double center_ray[3], const double ex[3], const double ey[3],
                              const double* theta_cos_sin, const double* phi_cos_sin, double* workspace,
                              int64_t workspace_len, double* stats_out, void* stream);
int rtpb_focus_sweep_variants_collimated(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                                         int32_t n_variants, int32_t dtype, int32_t device, int64_t n_groups,
                                         const double* group_params, const int32_t* group_variant,
                                         const double* group_frames, int64_t n_disps, int64_t nphis,
                                         const double* offsets, const double* phi_cos_sin, double* workspace,
                                         int64_t workspace_len, double* stats_out, void* stream);

/* The WAVEFRONT statistics over many systems: rtpb_wavefront_sweep / rtpb_wavefront_sweep_collimated with the systems
   in the call, as above.  There is no dtype argument: the calls are float64, as the wavefront statistics are.  The
   arguments after group_variant are those of rtpb_wavefront_sweep from n_thetas through refs (HOST, n_groups x 8), of
   rtpb_wavefront_sweep_collimated from group_frames through refs; stats_out (DEVICE, n_groups x 15).  Every group is
   swept on its own, with rtpb_trace's own surface steps.
   CONTRACT: a group's 15 sums are bit-identical to those rtpb_wavefront_sweep[_collimated] gives the same group, with
   the same reference, on a float64 plan created from its variant's descriptors -- whatever else the call holds.
   The checks, their order and the error codes are those of rtpb_focus_sweep_variants, with a NULL refs
   RTPB_E_INVALID; the short workspace is n_groups * ceil(rays per group / 256) * 15 doubles, and the upload counts the
   references and one word more:
       16 (n_thetas + nphis) + n_groups (8 (4 nsurf + 5) + 12) + 280 n_variants nsurf + 64 n_groups + 8
   (a collimated call: 72 n_groups more) against RTPB_MAX_VARIANT_UPLOAD. */
int rtpb_wavefront_sweep_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                                  int32_t n_variants, int32_t device, int64_t n_groups, const double* group_params,
                                  const int32_t* group_variant, int64_t n_thetas, int64_t nphis,
                                  const double center_ray[3], const double ex[3], const double ey[3],
                                  const double* theta_cos_sin, const double* phi_cos_sin, const double* refs,
                                  double* workspace, int64_t workspace_len, double* stats_out, void* stream);
int rtpb_wavefront_sweep_variants_collimated(const rtpb_surface* surfaces, int32_t nsurf,
                                             const rtpb_material* materials, int32_t n_variants, int32_t device,
                                             int64_t n_groups, const double* group_params,
                                             const int32_t* group_variant, const double* group_frames,
                                             int64_t n_disps, int64_t nphis, const double* offsets,
                                             const double* phi_cos_sin, const double* refs, double* workspace,
                                             int64_t workspace_len, double* stats_out, void* stream);

/* The FINAL RAYS of a few generated rays per group, each group through its own variant: the fan (beam) of every group
   is generated from the sweep's own source arguments, traced through the group's variant with rtpb_trace's own surface
   steps, phase kept, and every ray's final state is stored as 8 float64 {x, y, z, dx, dy, dz, phase, wavelength} to
   rays_out (DEVICE, n_groups x rays per group x 8, AOS), ray j = itheta + n_thetas * iphi (iphi + nphis * idisp) of
   group g at row g * rays per group + j.  Nothing else is written.  float64 only; no workspace.
   CONTRACT: a group's rows are bit-identical to rtpb_ray_fan_tables (rtpb_collimated_rays_tables) followed by
   rtpb_trace (final plane) on a float64 plan created from its variant's descriptors; a ray that dies on the way
   stores the row rtpb_trace stores for it.  With the tables of theta_max = 0, n_thetas = nphis = 1 (one zero offset,
   n_disps = nphis = 1) a group's one ray is its chief ray, the ray get_ray_fan(field, 0, 1, wavelength, center_ray)
   (get_collimated_rays(pt, 0, 1, wavelength, normal)) gives: the references of rtpb_wavefront_sweep_variants for all
   (variant, field, wavelength) groups come from one call.
   The checks and error codes are those of rtpb_focus_sweep_variants without a workspace (a NULL rays_out is
   RTPB_E_INVALID), the upload bound its own; more than 256 rays per group (one tile) is RTPB_E_LIMIT. */
int rtpb_final_rays_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                             int32_t n_variants, int32_t device, int64_t n_groups, const double* group_params,
                             const int32_t* group_variant, int64_t n_thetas, int64_t nphis,
                             const double center_ray[3], const double ex[3], const double ey[3],
                             const double* theta_cos_sin, const double* phi_cos_sin, double* rays_out, void* stream);
int rtpb_final_rays_variants_collimated(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                                        int32_t n_variants, int32_t device, int64_t n_groups,
                                        const double* group_params, const int32_t* group_variant,
                                        const double* group_frames, int64_t n_disps, int64_t nphis,
                                        const double* offsets, const double* phi_cos_sin, double* rays_out,
                                        void* stream);

/* ---- pupil-phase interpolation (scripts/2022_02_06_perfect_imaging_system_psf.py:90-105) */
/* A 2-D Delaunay triangulation with one value per vertex, in scipy.spatial.Delaunay's representation,
   plus a uniform cell index (CSR lists of the triangles whose bounding box meets each cell, in
   increasing triangle order).  All pointers are device pointers. */
typedef struct rtpb_triangulation {
    int64_t n_tri;
    const double* transform;    /* n_tri x 3 x 2: Delaunay.transform (2x2 inverse, then the offset row) */
    const int32_t* simplices;   /* n_tri x 3 vertex indices */
    const double* values;       /* value of each vertex */
    int32_t cells_x, cells_y;   /* cell (cx, cy) covers [x0 + cx*cell_w, +cell_w) x [y0 + cy*cell_h, +cell_h) */
    double x0, y0, cell_w, cell_h;
    const int32_t* cell_start;  /* cells_x*cells_y + 1 offsets into cell_tris; cell id = cy*cells_x + cx */
    const int32_t* cell_tris;
} rtpb_triangulation;

/* griddata(points, values, (xx, yy), method='linear') on the grid meshgrid(xs, ys) (point (iy, ix) =
   (xs[ix], ys[iy]), row-major), with scipy's LinearNDInterpolator arithmetic: the first triangle whose
   barycentric coordinates lie in [-eps, 1+eps] (eps = 100 DBL_EPSILON), c0/c1 from the transform and
   c2 = (1 - c0) - c1, value = ((0 + c0 v0) + c1 v1) + c2 v2; NaN outside the hull.  Optionally fused
   with the pupil field of the script: field = exp(i phase), 0 where phase is NaN or
   sqrt(x^2 + y^2) > radius.  phase_out (ny*nx doubles) and/or field_out (ny*nx interleaved complex
   doubles) may be NULL.  xs, ys: device arrays. */
int rtpb_grid_interpolate(int32_t device, const rtpb_triangulation* tri, const double* xs, int64_t nx,
                          const double* ys, int64_t ny, double radius, double* phase_out, double* field_out,
                          void* stream);

/* ---- distinct wavelengths of a device-resident bundle (keys of the plan's RTPB_TABLE materials) -- */
/* Replaces the host-side np.unique of the wavelength column that tabulated materials need
   (MAT:128-144 Ebaf11 and user Material.n are evaluated by the host at exactly these wavelengths).
   col: device pointer to the first wavelength, `stride` elements between consecutive rays (8 for an
   (N, 8) AoS bundle), n values of `dtype` (RTPB_F64 / RTPB_F32, widened exactly).  table: device buffer
   of `table_slots` uint64 (a power of two); max_keys <= table_slots / 2; count: one device uint32.
   Asynchronous on `stream`.  Afterwards the table holds the distinct keys as float64 bit patterns (all
   NaNs as one quiet-NaN key, -0.0 as +0.0) in arbitrary order, empty slots = all-ones; *count is the
   number of keys, or > max_keys when there are more (the caller then sorts instead). */
int rtpb_distinct_keys(int32_t device, const void* col, int32_t dtype, int64_t n, int64_t stride, uint64_t* table,
                       int32_t table_slots, int32_t max_keys, uint32_t* count, void* stream);

/* ---- tuning knobs (benchmarks / A-B tests; process-wide) ------------------------------------ */
/* "aos_staging": 1 (default) = AOS planes are written through a per-wave LDS tile so every global
   store instruction writes 1 KiB contiguous; 0 = direct 16-byte stores at the record stride.
   "nt_stores": 1 (default) = non-temporal global stores for the staged AOS tiles (the history is
   streamed out and never re-read by the kernel); 0 = default cache policy.
   "stage_input": 1 = also load AOS input records through the LDS tile (1 KiB per load instruction);
   0 (default) = 4 x 16-byte loads per lane.
   "host_chunk_mib": input + output bytes per pipelined chunk of rtpb_trace_host (default 128).
   "indexed_materials": 1 (default) = plans created from now on whose TABLE materials all share one
   key set (and that have no POLY6 material) also tabulate every other material at those keys, so the
   kernel reads n from LDS instead of evaluating Sellmeier dispersion per surface (bit-identical: the
   host evaluates the kernel's own material_n); 0 = evaluate per surface.
   "buffer_pool_buffers": freed history buffers kept mapped per device for reuse (default 1, 0..1024).
   "buffer_dead_va_limit": reserved virtual bytes of released buffer mappings (never reused) beyond which new
                           history buffers are plain hipMalloc allocations (default 32 TiB). */
int rtpb_set_tuning(const char* key, int64_t value);

/* ---- kernel timing (benchmarks) ------------------------------------------------------------- */
/* While enabled on the calling thread, every trace kernel this thread launches is bracketed by a pair
   of HIP events recorded on the kernel's own stream.  rtpb_timing_collect() waits for them and
   returns the summed kernel time (ms) and launch count since the last collect, then resets. */
int rtpb_timing_enable(int32_t on);
int rtpb_timing_collect(double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* RTPB_H */
