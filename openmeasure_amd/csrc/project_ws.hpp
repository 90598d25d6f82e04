// W-stationary projection kernel (project_ws.hip), internal to the library: tried first by project.hip's entry points.
#pragma once
#include "common.hpp"

// The field the projection can emit next to the basis (spr_project_field_*): x[v] = scale_f (Ur a_v) + rowmean for n_p
// coefficient vectors A (n_p x r, packed), written to out[v * ldo + row].  Needs center != 0 (the row means are the centre).
struct WsField {
  const double *scale;   // (n_features,) X_scl per feature
  const double *A;       // (n_p, r) coefficient vectors
  int32_t n_p;
  double *out;           // (n_p, ldo)
  int64_t ldo;
};

// SPR_OK when launched; SPR_E_UNSUPPORTED when the shape is outside its range (m not 64/128/192/256 packed and 16-byte
// aligned, r > 64, accumulate; with a field: n_p > SPR_FIELD_NF or r not a multiple of 16) -- the caller then launches the
// general kernel.  Other codes are errors.
// d_rownorm2 != NULL: the squared norms of the stored rows of Ur are written there as well (n_rows doubles).
// field != NULL: the field of those rows as well (see WsField).
template <typename TX, typename TU>
int spr_project_ws(const TX *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0, int64_t n_points,
                   int32_t n_features, int32_t center, const double *d_inv_scale, const double *d_rowmean,
                   const double *d_W, int32_t r, TU *d_Ur, int64_t ldu, int32_t accumulate,
                   double *d_rownorm2, hipStream_t st, const WsField *field = nullptr);
