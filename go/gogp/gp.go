// Package gogp is the drop-in replacement of bitbucket.org/dtolpin/gogp/gp for the
// hot path (Absorb / LML / Produce / Observe / Gradient), calling the MI355X HIP
// library through cgo.  NOT COMPILED IN THIS REPOSITORY'S CI: the build image has
// no Go toolchain; the same C ABI is exercised from Python (ctypes) and C++.
//
// Build:  CGO_CFLAGS="-I${REPO}/include" CGO_LDFLAGS="-L${REPO}/gogp_amd -lgogp_hip" go build ./go/gogp
package gogp

/*
#include <stdlib.h>
#include "gogp_hip.h"
*/
import "C"

import (
	"fmt"
	"math"
	"runtime"
	"sort"
	"unsafe"
)

// Kernel is the reference's kernel interface (gp/gp.go:14-17) plus the closed
// description the device path needs.  Kernels that cannot describe themselves
// (arbitrary Go code) must keep using the reference package.
type Kernel interface {
	Observe([]float64) float64
	NTheta() int
}

// DeviceKernel is implemented by similarity kernels that can run on the GPU.
type DeviceKernel interface {
	Kernel
	Terms() []Term
}

// EventKernel is optionally implemented by a DeviceKernel whose similarity is
// discounted across event boundaries (tutorial/events/kernel/kernel.go:14-44):
// Events() returns [from, to, discount] triples, EventAxis() the input dimension
// they lie on (0 for the reference's 1-D case).  The shim passes them to
// gogp_set_events.
type EventKernel interface {
	Events() [][]float64
	EventAxis() int
}

// DeviceNoise is implemented by noise kernels that can run on the GPU.
type DeviceNoise interface {
	Kernel
	NoiseDesc() (kind int, std, scale float64)
}

// Term mirrors gogp_term of include/gogp_hip.h.
type Term struct {
	Kind, ScaleIdx, LenIdx int
	ARD                    bool
	PeriodIdx              int
	PeriodMult             float64
}

// GP keeps the reference's exported fields (gp/gp.go:20-38).
type GP struct {
	NDim         int
	Simil, Noise Kernel

	ThetaSimil, ThetaNoise []float64
	X                      [][]float64
	Y                      []float64

	Parallel bool // accepted for compatibility; the device path is always parallel

	// Cached computations (gp/gp.go:34-36).  Alpha is refreshed by every Absorb / Observe;
	// the factor is fetched on demand by Factor() (n*n doubles over PCIe are not free).
	Alpha []float64 // K^-1 y

	h       *C.gogp_handle
	withObs bool
	lastLen int
	// X, Y are uploaded only when they changed.  Absorb and the full form of Observe assign
	// them; code that writes gp.X / gp.Y directly (the reference's tutorial does:
	// tutorial/tutorial.go:114-115) is detected by comparing the slice headers below, and
	// in-place edits of the same backing arrays must call Touch().
	dirty      bool
	nout       int // output columns of SetOutputs
	nbasis     int // basis columns of SetBasis
	sparseM    int // inducing points of SetSparse
	sparseT    int // output columns of SetSparseOutputs
	upX        *[]float64 // &gp.X[0] at the time of the last upload
	upY        *float64   // &gp.Y[0] at the time of the last upload
	upN        int
}

// Touch marks X / Y as modified in place: the next Absorb / Observe uploads them again.
func (gp *GP) Touch() { gp.dirty = true }

func (gp *GP) handle() *C.gogp_handle {
	if gp.h != nil {
		return gp.h
	}
	sim, ok := gp.Simil.(DeviceKernel)
	if !ok {
		panic("gogp: Simil does not implement DeviceKernel; use the reference package for arbitrary Go kernels")
	}
	var d C.gogp_desc
	d.ndim = C.int32_t(gp.NDim)
	terms := sim.Terms()
	d.nterms = C.int32_t(len(terms))
	d.ntheta_simil = C.int32_t(sim.NTheta())
	for i, t := range terms {
		ct := &d.terms[i]
		ct.kind, ct.scale_idx, ct.len_idx = C.int32_t(t.Kind), C.int32_t(t.ScaleIdx), C.int32_t(t.LenIdx)
		if t.ARD {
			ct.ard = 1
		}
		ct.period_idx, ct.period_mult = C.int32_t(t.PeriodIdx), C.double(t.PeriodMult)
	}
	if gp.Noise == nil { // gp/gp.go:45-48: ConstantNoise(1e-5)
		d.noise_kind, d.noise_std = C.GOGP_NOISE_CONSTANT, 1e-5
	} else {
		dn, ok := gp.Noise.(DeviceNoise)
		if !ok {
			panic("gogp: Noise does not implement DeviceNoise; use the reference package for arbitrary Go kernels")
		}
		kind, std, scale := dn.NoiseDesc()
		d.noise_kind, d.noise_std, d.noise_scale = C.int32_t(kind), C.double(std), C.double(scale)
	}
	if rc := C.gogp_create(&d, -1, &gp.h); rc != C.GOGP_OK {
		panic(fmt.Sprintf("gogp_create: %s", C.GoString(C.gogp_last_error(nil))))
	}
	runtime.SetFinalizer(gp, func(g *GP) { C.gogp_destroy(g.h) })
	if ek, ok := gp.Simil.(EventKernel); ok && len(ek.Events()) > 0 {
		evs := ek.Events()
		flat := make([]float64, 0, 3*len(evs))
		for _, e := range evs {
			if len(e) != 3 {
				panic("gogp: an event is [from, to, discount]")
			}
			flat = append(flat, e...)
		}
		if rc := C.gogp_set_events(gp.h, dptr(flat), C.int(len(evs)), C.int(ek.EventAxis())); rc != C.GOGP_OK {
			panic(fmt.Sprintf("gogp_set_events: %s", C.GoString(C.gogp_last_error(gp.h))))
		}
	}
	gp.dirty = true
	return gp.h
}

func (gp *GP) err(rc C.int) error {
	if rc == C.GOGP_OK {
		return nil
	}
	return fmt.Errorf("gogp_hip: %s", C.GoString(C.gogp_last_error(gp.h)))
}

func dptr(s []float64) *C.double {
	if len(s) == 0 {
		return nil
	}
	return (*C.double)(unsafe.Pointer(&s[0]))
}

// changed reports whether gp.X / gp.Y were re-assigned since the last upload.
func (gp *GP) changed() bool {
	if gp.dirty || len(gp.X) != gp.upN || len(gp.Y) != gp.upN {
		return true
	}
	if gp.upN == 0 {
		return false
	}
	return &gp.X[0] != gp.upX || &gp.Y[0] != gp.upY
}

// pushData packs X ([][]float64, not contiguous) row-major and copies X, Y to the device --
// only when they changed: a hyperparameter step must not pay an O(N*D) host-to-device copy
// and a drain of the device streams.
func (gp *GP) pushData() error {
	h := gp.handle()
	if !gp.changed() {
		return nil
	}
	n := len(gp.X)
	if len(gp.Y) != n {
		return fmt.Errorf("gogp: len(X) != len(Y)")
	}
	flat := make([]float64, n*gp.NDim)
	for i, row := range gp.X {
		copy(flat[i*gp.NDim:], row)
	}
	if err := gp.err(C.gogp_set_data(h, dptr(flat), dptr(gp.Y), C.int64_t(n))); err != nil {
		return err
	}
	gp.dirty, gp.upN = false, n
	if n > 0 {
		gp.upX, gp.upY = &gp.X[0], &gp.Y[0]
	}
	return nil
}

func (gp *GP) defaults() { // gp/gp.go:45-57
	if len(gp.ThetaSimil) == 0 {
		gp.ThetaSimil = make([]float64, gp.Simil.NTheta())
	}
	nn := 0
	if gp.Noise != nil {
		nn = gp.Noise.NTheta()
	}
	if len(gp.ThetaNoise) == 0 {
		gp.ThetaNoise = make([]float64, nn)
	}
}

// SetNoiseVariances sets known noise variances, one per observation: K = k(X, X) + sigma^2(theta) I +
// diag(v), every v[i] finite and >= 0 (gogp_set_noise_variances; no reference counterpart).  nil
// clears them.  Stored results are dropped: Absorb or Observe again.  The variances belong to the
// data: re-assigning X / Y (and so Absorb) clears them, AppendNoisy / Append and Remove carry them.
func (gp *GP) SetNoiseVariances(v []float64) error {
	if v == nil {
		if gp.changed() {
			return nil // nothing of the current data is on the device yet
		}
		return gp.err(C.gogp_set_noise_variances(gp.handle(), nil, 0))
	}
	if len(v) != len(gp.Y) {
		return fmt.Errorf("gogp: SetNoiseVariances: one variance per observation")
	}
	if err := gp.pushData(); err != nil {
		return err
	}
	return gp.err(C.gogp_set_noise_variances(gp.handle(), dptr(v), C.int64_t(len(v))))
}

// NoiseVariances returns what the device holds for the current observations (zeros when none are set).
func (gp *GP) NoiseVariances() ([]float64, error) {
	if gp.changed() {
		return make([]float64, len(gp.Y)), nil
	}
	v := make([]float64, int(C.gogp_n(gp.handle())))
	if err := gp.err(C.gogp_get_noise_variances(gp.handle(), dptr(v))); err != nil {
		return nil, err
	}
	return v, nil
}

// NoiseVariancesGradient returns dLML/dv[i] = 1/2 (Alpha[i]^2 - [K^-1]_ii) at the current parameters
// and variances (gogp_noise_variances_gradient); also with no variances set.
func (gp *GP) NoiseVariancesGradient() ([]float64, error) {
	dv := make([]float64, int(C.gogp_n(gp.handle())))
	if err := gp.err(C.gogp_noise_variances_gradient(gp.handle(), dptr(dv))); err != nil {
		return nil, err
	}
	return dv, nil
}

// AbsorbNoisy is Absorb with the observations' noise variances v (SetNoiseVariances).
func (gp *GP) AbsorbNoisy(x [][]float64, y, v []float64) error {
	return gp.absorb(x, y, v)
}

// Absorb absorbs observations into the process (gp/gp.go:80-87).  Noise variances of the previous
// data are cleared.
func (gp *GP) Absorb(x [][]float64, y []float64) error {
	return gp.absorb(x, y, nil)
}

func (gp *GP) absorb(x [][]float64, y, v []float64) (err error) {
	gp.defaults()
	gp.X, gp.Y = x, y
	gp.dirty = true // also when the same slices come again: the upload drops the old variances
	if err = gp.pushData(); err != nil {
		return err
	}
	if v != nil {
		if err = gp.SetNoiseVariances(v); err != nil {
			return err
		}
	}
	tn := gp.ThetaNoise
	if len(tn) == 0 {
		tn = []float64{0}
	}
	rc := C.gogp_absorb(gp.handle(), dptr(gp.ThetaSimil), dptr(tn))
	if rc != C.GOGP_OK && rc != C.GOGP_ECOND {
		return gp.err(rc) // gp/gp.go:228-230
	}
	if err = gp.fetchState(); err != nil {
		return err
	}
	return gp.err(rc) // GOGP_ECOND: gonum's Condition error, returned as gp/gp.go:233-236 does
}

// Append appends observations to the absorbed ones at the parameters of the last Absorb / Observe
// (gogp_append): the state Absorb on all observations would leave, without a new factorisation.
// No reference counterpart (tutorial/tutorial.go:118-142 refactorises every step).  An empty process
// absorbs them at ThetaSimil / ThetaNoise.  When the enlarged matrix is not positive definite the
// error is returned and the process is as it was.
func (gp *GP) Append(x [][]float64, y []float64) error {
	return gp.AppendNoisy(x, y, nil)
}

// AppendNoisy is Append with the new observations' noise variances v (gogp_append_noisy); nil: zeros.
// With v on a process without variances the old rows get zeros.
func (gp *GP) AppendNoisy(x [][]float64, y, v []float64) (err error) {
	gp.defaults()
	if len(x) != len(y) || (v != nil && len(v) != len(y)) {
		return fmt.Errorf("gogp: len(x) != len(y)")
	}
	if len(gp.Y) == 0 {
		if err = gp.pushData(); err != nil {
			return err
		}
		tn := gp.ThetaNoise
		if len(tn) == 0 {
			tn = []float64{0}
		}
		if err = gp.err(C.gogp_absorb(gp.handle(), dptr(gp.ThetaSimil), dptr(tn))); err != nil {
			return err
		}
	} else if gp.changed() {
		return fmt.Errorf("gogp: Append: X / Y were assigned since the last Absorb / Observe; Absorb them")
	}
	m := len(y)
	if m == 0 {
		return nil
	}
	flat := make([]float64, m*gp.NDim)
	for i, row := range x {
		copy(flat[i*gp.NDim:], row)
	}
	var rc C.int
	if v == nil {
		rc = C.gogp_append(gp.handle(), dptr(flat), dptr(y), C.int64_t(m))
	} else {
		rc = C.gogp_append_noisy(gp.handle(), dptr(flat), dptr(y), dptr(v), C.int64_t(m))
	}
	if rc != C.GOGP_OK && rc != C.GOGP_ECOND {
		return gp.err(rc)
	}
	// the device holds the grown data: X / Y follow without a new upload
	gp.X = append(gp.X[:len(gp.X):len(gp.X)], x...)
	gp.Y = append(gp.Y[:len(gp.Y):len(gp.Y)], y...)
	gp.dirty, gp.upN = false, len(gp.Y)
	gp.upX, gp.upY = &gp.X[0], &gp.Y[0]
	if err = gp.fetchState(); err != nil {
		return err
	}
	return gp.err(rc)
}

// Remove removes the observations with the indices idx (any order, no duplicates) from the absorbed
// ones (gogp_remove): the state Absorb on the kept rows would leave, without a new factorisation and
// at the parameters of the last Absorb / Observe.  No reference counterpart; the counterpart of
// Append, with which a bounded window slides: Remove([]int{0}), then Append(new).
func (gp *GP) Remove(idx []int) (err error) {
	gp.defaults()
	s := make([]int64, len(idx))
	for i, v := range idx {
		s[i] = int64(v)
	}
	sort.Slice(s, func(a, b int) bool { return s[a] < s[b] })
	for j, v := range s {
		if v < 0 || v >= int64(len(gp.Y)) || (j > 0 && v == s[j-1]) {
			return fmt.Errorf("gogp: Remove: index %d out of range or repeated", v)
		}
	}
	if gp.changed() {
		return fmt.Errorf("gogp: Remove: X / Y were assigned since the last Absorb / Observe; Absorb them")
	}
	if len(s) == 0 {
		return nil
	}
	rc := C.gogp_remove(gp.handle(), (*C.int64_t)(unsafe.Pointer(&s[0])), C.int64_t(len(s)))
	if rc != C.GOGP_OK && rc != C.GOGP_ECOND {
		return gp.err(rc)
	}
	// the device holds the compacted data: X / Y follow without a new upload
	k, j := 0, 0
	X, Y := make([][]float64, 0, len(gp.Y)-len(s)), make([]float64, 0, len(gp.Y)-len(s))
	for i := range gp.Y {
		if j < len(s) && s[j] == int64(i) {
			j++
			continue
		}
		X, Y = append(X, gp.X[i]), append(Y, gp.Y[i])
		k++
	}
	gp.X, gp.Y = X, Y
	gp.dirty, gp.upN = false, k
	if k > 0 {
		gp.upX, gp.upY = &gp.X[0], &gp.Y[0]
	} else {
		gp.upX, gp.upY = nil, nil
	}
	if err = gp.fetchState(); err != nil {
		return err
	}
	return gp.err(rc)
}

// Factor returns the lower Cholesky factor, row-major n x n (gonum's mat.Cholesky keeps
// U = L^T: gp.GP.L of the reference, gp/gp.go:35).
func (gp *GP) Factor() ([]float64, error) {
	n := int(C.gogp_n(gp.handle()))
	L := make([]float64, n*n)
	if err := gp.err(C.gogp_get_factor(gp.h, dptr(L))); err != nil {
		return nil, err
	}
	return L, nil
}

func (gp *GP) fetchState() error {
	n := int(C.gogp_n(gp.h))
	gp.Alpha = make([]float64, n)
	return gp.err(C.gogp_get_alpha(gp.h, dptr(gp.Alpha)))
}

// LML computes log marginal likelihood (gp/gp.go:244-253).
func (gp *GP) LML() float64 {
	var v C.double
	if err := gp.err(C.gogp_lml(gp.handle(), &v)); err != nil {
		panic(err)
	}
	return float64(v)
}

// Produce computes predictions (gp/gp.go:258-360).
func (gp *GP) Produce(x [][]float64) (mu, sigma []float64, err error) {
	gp.defaults()
	m := len(x)
	flat := make([]float64, m*gp.NDim)
	for i, row := range x {
		copy(flat[i*gp.NDim:], row)
	}
	mu, sigma = make([]float64, m), make([]float64, m)
	if err = gp.err(C.gogp_produce(gp.handle(), dptr(flat), C.int64_t(m), dptr(mu), dptr(sigma))); err != nil {
		return nil, nil, err // gp/gp.go:338-340
	}
	return mu, sigma, nil
}

// ProduceGradient computes predictions and their derivatives with respect to
// the test points: dmu[i*NDim+d] = d mu_i / d x[i][d], dsigma likewise (no
// reference counterpart).
func (gp *GP) ProduceGradient(x [][]float64) (mu, sigma, dmu, dsigma []float64, err error) {
	gp.defaults()
	m := len(x)
	flat := make([]float64, m*gp.NDim)
	for i, row := range x {
		copy(flat[i*gp.NDim:], row)
	}
	mu, sigma = make([]float64, m), make([]float64, m)
	dmu, dsigma = make([]float64, m*gp.NDim), make([]float64, m*gp.NDim)
	if err = gp.err(C.gogp_produce_gradient(gp.handle(), dptr(flat), C.int64_t(m), dptr(mu), dptr(sigma), dptr(dmu), dptr(dsigma))); err != nil {
		return nil, nil, nil, nil, err
	}
	return mu, sigma, dmu, dsigma, nil
}

// ProduceCovariance computes the predicted means and the joint covariance of
// the latent function at the test points: cov[i*m+j], symmetric, no noise term
// (no reference counterpart).
func (gp *GP) ProduceCovariance(x [][]float64) (mu, cov []float64, err error) {
	gp.defaults()
	m := len(x)
	flat := make([]float64, m*gp.NDim)
	for i, row := range x {
		copy(flat[i*gp.NDim:], row)
	}
	mu, cov = make([]float64, m), make([]float64, m*m)
	if err = gp.err(C.gogp_produce_covariance(gp.handle(), dptr(flat), C.int64_t(m), dptr(mu), dptr(cov))); err != nil {
		return nil, nil, err
	}
	return mu, cov, nil
}

// Likelihoods of LaplaceObserve (enum gogp_lik_kind).
const (
	BernoulliLogit = int(C.GOGP_LIK_BERNOULLI_LOGIT) // Y in {0, 1}
	PoissonLog     = int(C.GOGP_LIK_POISSON_LOG)     // Y: counts
)

// ErrNoConvergence is returned by LaplaceObserve when Newton's iteration did
// not reach the tolerance; the last iterate is stored and its value returned.
var ErrNoConvergence = fmt.Errorf("gogp_hip: laplace: Newton did not reach the tolerance")

// LaplaceObserve computes the approximate log marginal likelihood of Y under
// the likelihood lik at x = log theta by the Laplace approximation around the
// mode found by a damped Newton iteration (no reference counterpart). It drops
// the regression state: Gradient, Produce and the rest need a new Absorb or
// Observe. Unlike Observe, whose signature is the reference's and which must
// panic where the reference does, this call has an error result: GOGP_ECOND
// and GOGP_ENOCONV both come back as errors (ErrNoConvergence for the latter)
// together with the stored value, as Absorb returns GOGP_ECOND; nothing panics.
func (gp *GP) LaplaceObserve(x []float64, lik int) (float64, error) {
	gp.defaults()
	if err := gp.pushData(); err != nil {
		return 0, err
	}
	gp.withObs = false
	var z C.double
	rc := C.gogp_laplace_observe(gp.handle(), C.int32_t(lik), dptr(x), C.int64_t(len(x)), &z)
	if rc == C.GOGP_OK || rc == C.GOGP_ECOND || rc == C.GOGP_ENOCONV {
		ns := len(gp.ThetaSimil)
		for i := range gp.ThetaSimil {
			gp.ThetaSimil[i] = math.Exp(x[i])
		}
		for i := range gp.ThetaNoise {
			gp.ThetaNoise[i] = math.Exp(x[ns+i])
		}
	}
	if rc == C.GOGP_ENOCONV {
		return float64(z), ErrNoConvergence
	}
	return float64(z), gp.err(rc)
}

// LaplaceGradient computes the gradient of LaplaceObserve with respect to the
// log-transformed hyperparameters, the movement of the mode included.
func (gp *GP) LaplaceGradient() ([]float64, error) {
	gp.defaults()
	g := make([]float64, len(gp.ThetaSimil)+len(gp.ThetaNoise))
	if err := gp.err(C.gogp_laplace_gradient(gp.handle(), dptr(g), C.int64_t(len(g)))); err != nil {
		return nil, err
	}
	return g, nil
}

// LaplaceMode returns the latent values f and a = K^-1 f at the mode and the
// Newton steps the last LaplaceObserve took.
func (gp *GP) LaplaceMode() (f, a []float64, iterations int, err error) {
	n := int(C.gogp_n(gp.handle()))
	f, a = make([]float64, n), make([]float64, n)
	var it C.int32_t
	if err = gp.err(C.gogp_laplace_get_mode(gp.handle(), dptr(f), dptr(a), &it)); err != nil {
		return nil, nil, 0, err
	}
	return f, a, int(it), nil
}

// LaplaceProduce computes the latent mean and standard deviation (no noise, as
// Produce) and the response-scale prediction at the test points: E[y*] for
// PoissonLog, P(y* = 1) for BernoulliLogit.
func (gp *GP) LaplaceProduce(x [][]float64) (mu, sigma, mean []float64, err error) {
	m := len(x)
	flat := make([]float64, m*gp.NDim)
	for i, row := range x {
		copy(flat[i*gp.NDim:], row)
	}
	mu, sigma, mean = make([]float64, m), make([]float64, m), make([]float64, m)
	rc := C.gogp_laplace_produce(gp.handle(), dptr(flat), C.int64_t(m), dptr(mu), dptr(sigma), dptr(mean))
	if err = gp.err(rc); err != nil {
		return nil, nil, nil, err
	}
	return mu, sigma, mean, nil
}

// LOO computes the leave-one-out cross-validation predictions at the current
// parameters: mean, standard deviation and log density of every observation
// under the process fitted to the others, and the sum of the log densities (no
// reference counterpart).
func (gp *GP) LOO() (mu, sigma, logp []float64, total float64, err error) {
	gp.defaults()
	n := int(C.gogp_n(gp.handle()))
	mu, sigma, logp = make([]float64, n), make([]float64, n), make([]float64, n)
	var t C.double
	if err = gp.err(C.gogp_loo(gp.handle(), dptr(mu), dptr(sigma), dptr(logp), &t)); err != nil {
		return nil, nil, nil, 0, err
	}
	return mu, sigma, logp, float64(t), nil
}

// LOOGradient computes the gradient of the LOO score with respect to the
// log-transformed hyperparameters (no reference counterpart).
func (gp *GP) LOOGradient() ([]float64, error) {
	gp.defaults()
	g := make([]float64, len(gp.ThetaSimil)+len(gp.ThetaNoise))
	if err := gp.err(C.gogp_loo_gradient(gp.handle(), dptr(g), C.int64_t(len(g)))); err != nil {
		return nil, err
	}
	return g, nil
}

// Blocks returns start for BlockCV: n rows in consecutive blocks of length
// rows, the last one shorter where length does not divide n.
func Blocks(n, length int) []int64 {
	start := []int64{}
	for s := 0; s < n && length > 0; s += length {
		start = append(start, int64(s))
	}
	return append(start, int64(n))
}

// BlockCV computes the leave-block-out cross-validation predictions at the
// current parameters (gogp_blockcv): the rows are cut into the consecutive
// blocks [start[f], start[f+1]), start[0] = 0, start[F] = n, 1 .. 128 rows
// each, and every block is predicted jointly by the process fitted to all the
// other blocks.  mu, sigma: per row; logp: the joint log density per block;
// total: their sum (no reference counterpart).  Folds that are not contiguous:
// permute the rows before assigning X / Y.
func (gp *GP) BlockCV(start []int64) (mu, sigma, logp []float64, total float64, err error) {
	gp.defaults()
	if len(start) == 0 {
		return nil, nil, nil, 0, fmt.Errorf("gogp: BlockCV: start needs F + 1 entries")
	}
	n, f := int(C.gogp_n(gp.handle())), len(start)-1
	mu, sigma, logp = make([]float64, n), make([]float64, n), make([]float64, f)
	var t C.double
	rc := C.gogp_blockcv(gp.handle(), (*C.int64_t)(unsafe.Pointer(&start[0])), C.int64_t(f), dptr(mu), dptr(sigma), dptr(logp), &t)
	if err = gp.err(rc); err != nil {
		return nil, nil, nil, 0, err
	}
	return mu, sigma, logp, float64(t), nil
}

// BlockCVGradient computes the gradient of the BlockCV score with respect to
// the log-transformed hyperparameters (no reference counterpart).
func (gp *GP) BlockCVGradient(start []int64) ([]float64, error) {
	gp.defaults()
	if len(start) == 0 {
		return nil, fmt.Errorf("gogp: BlockCVGradient: start needs F + 1 entries")
	}
	g := make([]float64, len(gp.ThetaSimil)+len(gp.ThetaNoise))
	rc := C.gogp_blockcv_gradient(gp.handle(), (*C.int64_t)(unsafe.Pointer(&start[0])), C.int64_t(len(start)-1), dptr(g), C.int64_t(len(g)))
	if err := gp.err(rc); err != nil {
		return nil, err
	}
	return g, nil
}

// SetOutputs gives the process T output columns (y row-major n x T, n =
// len(gp.Y), T <= 128) observed at its inputs and sharing its kernel and
// hyperparameters; they are evaluated on one factorisation (no reference
// counterpart).  Pending X / Y are uploaded first.  T == 0 clears them; whatever
// replaces or resizes the data drops them.
func (gp *GP) SetOutputs(y []float64, T int) error {
	gp.defaults()
	if T == 0 {
		gp.nout = 0
		return gp.err(C.gogp_multi_set_outputs(gp.handle(), nil, 0, 0))
	}
	if err := gp.pushData(); err != nil {
		return err
	}
	if T < 0 || len(y) != len(gp.Y)*T {
		return fmt.Errorf("len(y)")
	}
	p := dptr(y)
	var none C.double
	if p == nil {
		p = &none
	}
	if err := gp.err(C.gogp_multi_set_outputs(gp.handle(), p, C.int64_t(len(gp.Y)), C.int32_t(T))); err != nil {
		return err
	}
	gp.nout = T
	return nil
}

// MultiLML computes the log marginal likelihood of every output column of
// SetOutputs at the current parameters, and their sum.
func (gp *GP) MultiLML() (total float64, lml []float64, err error) {
	gp.defaults()
	lml = make([]float64, gp.nout)
	var t C.double
	if err = gp.err(C.gogp_multi_lml(gp.handle(), &t, dptr(lml))); err != nil {
		return 0, nil, err
	}
	return float64(t), lml, nil
}

// MultiGradient computes the gradient of that sum with respect to the
// log-transformed hyperparameters.
func (gp *GP) MultiGradient() ([]float64, error) {
	gp.defaults()
	g := make([]float64, len(gp.ThetaSimil)+len(gp.ThetaNoise))
	if err := gp.err(C.gogp_multi_gradient(gp.handle(), dptr(g), C.int64_t(len(g)))); err != nil {
		return nil, err
	}
	return g, nil
}

// MultiAlpha returns A = K^-1 Y of the output columns, row-major n x T.
func (gp *GP) MultiAlpha() ([]float64, error) {
	gp.defaults()
	n := int(C.gogp_n(gp.handle()))
	a := make([]float64, n*gp.nout+1)
	if err := gp.err(C.gogp_multi_get_alpha(gp.handle(), dptr(a))); err != nil {
		return nil, err
	}
	return a[:n*gp.nout], nil
}

// MultiProduce computes the predictive means of every output column at the
// test points (row-major len(x) x T) and the standard deviation they share.
func (gp *GP) MultiProduce(x [][]float64) (mu, sigma []float64, err error) {
	gp.defaults()
	m := len(x)
	flat := make([]float64, m*gp.NDim)
	for i, row := range x {
		copy(flat[i*gp.NDim:], row)
	}
	buf, sigma := make([]float64, m*gp.nout+1), make([]float64, m)
	if err = gp.err(C.gogp_multi_produce(gp.handle(), dptr(flat), C.int64_t(m), dptr(buf), dptr(sigma))); err != nil {
		return nil, nil, err
	}
	return buf[:m*gp.nout], sigma, nil
}

// SetBasis gives the process the basis functions of a mean h(x)^T beta (h
// row-major n x p, n = len(gp.Y), p <= 64, p < n) whose coefficients are
// integrated out under a flat prior (Rasmussen & Williams section 2.7; no
// reference counterpart).  Pending X / Y are uploaded first.  p == 0 clears the
// basis; whatever replaces or resizes the data drops it.
func (gp *GP) SetBasis(h []float64, p int) error {
	gp.defaults()
	if p == 0 {
		gp.nbasis = 0
		return gp.err(C.gogp_basis_set(gp.handle(), nil, 0, 0))
	}
	if err := gp.pushData(); err != nil {
		return err
	}
	if p < 0 || len(h) != len(gp.Y)*p {
		return fmt.Errorf("gogp: len(h) = %d, want %d x %d", len(h), len(gp.Y), p)
	}
	if err := gp.err(C.gogp_basis_set(gp.handle(), dptr(h), C.int64_t(len(gp.Y)), C.int32_t(p))); err != nil {
		return err
	}
	gp.nbasis = p
	return nil
}

// BasisLML computes the log marginal likelihood with the coefficients of the
// mean integrated out, at the current parameters.
func (gp *GP) BasisLML() (float64, error) {
	gp.defaults()
	var v C.double
	if err := gp.err(C.gogp_basis_lml(gp.handle(), &v)); err != nil {
		return 0, err
	}
	return float64(v), nil
}

// BasisGradient computes the gradient of BasisLML with respect to the
// log-transformed hyperparameters.
func (gp *GP) BasisGradient() ([]float64, error) {
	gp.defaults()
	g := make([]float64, len(gp.ThetaSimil)+len(gp.ThetaNoise))
	if err := gp.err(C.gogp_basis_gradient(gp.handle(), dptr(g), C.int64_t(len(g)))); err != nil {
		return nil, err
	}
	return g, nil
}

// BasisBeta returns the estimate of the mean's coefficients and its covariance
// (H^T K^-1 H)^-1, row-major p x p.
func (gp *GP) BasisBeta() (beta, cov []float64, err error) {
	gp.defaults()
	p := gp.nbasis
	beta, cov = make([]float64, p+1), make([]float64, p*p+1)
	if err = gp.err(C.gogp_basis_get_beta(gp.handle(), dptr(beta), dptr(cov))); err != nil {
		return nil, nil, err
	}
	return beta[:p], cov[:p*p], nil
}

// BasisAlpha returns K^-1 (y - H beta).
func (gp *GP) BasisAlpha() ([]float64, error) {
	gp.defaults()
	n := int(C.gogp_n(gp.handle()))
	a := make([]float64, n+1)
	if err := gp.err(C.gogp_basis_get_alpha(gp.handle(), dptr(a))); err != nil {
		return nil, err
	}
	return a[:n], nil
}

// BasisProduce computes the predictive mean and standard deviation at the test
// points x whose basis functions are the rows of hz (row-major len(x) x p):
// Produce's mean plus the mean's contribution, the deviation widened by the
// uncertainty of the coefficients.
func (gp *GP) BasisProduce(x [][]float64, hz []float64) (mu, sigma []float64, err error) {
	gp.defaults()
	m := len(x)
	if len(hz) != m*gp.nbasis {
		return nil, nil, fmt.Errorf("gogp: len(hz) = %d, want %d x %d", len(hz), m, gp.nbasis)
	}
	flat := make([]float64, m*gp.NDim+1)
	for i, row := range x {
		copy(flat[i*gp.NDim:], row)
	}
	hbuf := append(append([]float64{}, hz...), 0)
	mu, sigma = make([]float64, m+1), make([]float64, m+1)
	if err = gp.err(C.gogp_basis_produce(gp.handle(), dptr(flat), dptr(hbuf), C.int64_t(m), dptr(mu), dptr(sigma))); err != nil {
		return nil, nil, err
	}
	return mu[:m], sigma[:m], nil
}

// SetSparse gives the process the data of the inducing-point approximation
// (no reference counterpart): N observations x (row-major N x NDim), y and M <=
// 4096 inducing points u (row-major M x NDim), kept on the device beside X / Y,
// which they do not touch.  An empty u clears them.
func (gp *GP) SetSparse(x, y, u []float64) error {
	gp.defaults()
	gp.sparseM = 0
	gp.sparseT = 0 // (the library drops the outputs of SetSparseOutputs with the data)
	if len(u) == 0 {
		return gp.err(C.gogp_sparse_set_data(gp.handle(), nil, nil, 0, nil, 0))
	}
	if len(x) != len(y)*gp.NDim || len(u)%gp.NDim != 0 {
		return fmt.Errorf("len(x), len(u)")
	}
	if err := gp.err(C.gogp_sparse_set_data(gp.handle(), dptr(x), dptr(y), C.int64_t(len(y)), dptr(u), C.int64_t(len(u)/gp.NDim))); err != nil {
		return err
	}
	gp.sparseM = len(u) / gp.NDim
	return nil
}

// SparseObserve computes the collapsed variational bound of Titsias (2009) of
// the sparse data at x = log theta: a lower bound of its log marginal
// likelihood at O(N M^2).
func (gp *GP) SparseObserve(x []float64) (float64, error) {
	gp.defaults()
	var b C.double
	if err := gp.err(C.gogp_sparse_observe(gp.handle(), dptr(x), C.int64_t(len(x)), &b)); err != nil {
		return float64(b), err
	}
	return float64(b), nil
}

// SparseGradient computes the gradient of that bound with respect to the
// log-transformed hyperparameters, at the parameters of the last SparseObserve.
func (gp *GP) SparseGradient() ([]float64, error) {
	gp.defaults()
	g := make([]float64, len(gp.ThetaSimil)+len(gp.ThetaNoise))
	if err := gp.err(C.gogp_sparse_gradient(gp.handle(), dptr(g), C.int64_t(len(g)))); err != nil {
		return nil, err
	}
	return g, nil
}

// SetInducing replaces the inducing points of SetSparse by u (row-major
// M x NDim, the same M) and nothing else: x, y and every device buffer stay.
// SparseObserve has to follow before a gradient or a forecast.
func (gp *GP) SetInducing(u []float64) error {
	gp.defaults()
	if len(u) == 0 || len(u)%gp.NDim != 0 {
		return fmt.Errorf("len(u)")
	}
	return gp.err(C.gogp_sparse_set_inducing(gp.handle(), dptr(u), C.int64_t(len(u)/gp.NDim)))
}

// SelectInducing chooses at most m inducing points among the rows of x
// (row-major N x NDim) at logtheta by greedy conditional-variance selection:
// a partial Cholesky factorisation of k(x, x) with diagonal pivoting (no
// reference counterpart; the noise does not enter).  It stops once no residual
// variance exceeds tol (tol < 0: the jitter 10^"sparse_jitter_log10"), so idx
// (the rows in pick order), u (= x[idx], row-major) and pivots (the residual
// variances at the picks) hold the points taken, m at most; trace is the
// trace term t0 - tr Qff of the bound for them.  x == nil selects among the
// rows of the sparse data already on the device (SetSparse), without sending
// them again.  Nothing of the process's state changes.
func (gp *GP) SelectInducing(logtheta, x []float64, m int, tol float64) (idx []int64, u, pivots []float64, trace float64, err error) {
	gp.defaults()
	if len(x)%gp.NDim != 0 {
		return nil, nil, nil, 0, fmt.Errorf("len(x)")
	}
	cnt := m
	if cnt < 1 {
		cnt = 1
	}
	idx, pivots, u = make([]int64, cnt), make([]float64, cnt), make([]float64, cnt*gp.NDim)
	var taken C.int64_t
	var tr C.double
	ip := (*C.int64_t)(unsafe.Pointer(&idx[0]))
	var rc C.int
	if x == nil {
		rc = C.gogp_sparse_select_inducing_resident(gp.handle(), dptr(logtheta), C.int64_t(len(logtheta)), C.int64_t(m),
			C.double(tol), ip, dptr(pivots), dptr(u), &taken, &tr)
	} else {
		rc = C.gogp_sparse_select_inducing(gp.handle(), dptr(logtheta), C.int64_t(len(logtheta)), dptr(x),
			C.int64_t(len(x)/gp.NDim), C.int64_t(m), C.double(tol), ip, dptr(pivots), dptr(u), &taken, &tr)
	}
	if err = gp.err(rc); err != nil {
		return nil, nil, nil, 0, err
	}
	k := int(taken)
	return idx[:k], u[:k*gp.NDim], pivots[:k], float64(tr), nil
}

// SparseGradientInducing computes SparseGradient and, from the same pass over
// the data, the derivative of the bound in the inducing points of SetSparse
// (row-major M x NDim).
func (gp *GP) SparseGradientInducing() (grad, dU []float64, err error) {
	gp.defaults()
	if gp.sparseM < 1 {
		return nil, nil, fmt.Errorf("SparseGradientInducing before SetSparse")
	}
	grad = make([]float64, len(gp.ThetaSimil)+len(gp.ThetaNoise))
	dU = make([]float64, gp.sparseM*gp.NDim)
	if err = gp.err(C.gogp_sparse_gradient_inducing(gp.handle(), dptr(grad), C.int64_t(len(grad)), dptr(dU))); err != nil {
		return nil, nil, err
	}
	return grad, dU, nil
}

// SparseProduce computes the predictive mean and standard deviation of the
// sparse approximation at the test points (latent and unclamped, as Produce).
func (gp *GP) SparseProduce(x [][]float64) (mu, sigma []float64, err error) {
	gp.defaults()
	m := len(x)
	flat := make([]float64, m*gp.NDim)
	for i, row := range x {
		copy(flat[i*gp.NDim:], row)
	}
	mu, sigma = make([]float64, m), make([]float64, m)
	if err = gp.err(C.gogp_sparse_produce(gp.handle(), dptr(flat), C.int64_t(m), dptr(mu), dptr(sigma))); err != nil {
		return nil, nil, err
	}
	return mu, sigma, nil
}

// SetSparseOutputs gives the sparse data nout <= 128 output columns observed
// at the inputs of SetSparse (no reference counterpart): yt is row-major
// N x nout with the N of SetSparse and stays on the device as given.  nout == 0
// clears them; SetSparse drops them, SetInducing keeps them.
func (gp *GP) SetSparseOutputs(yt []float64, nout int) error {
	gp.defaults()
	gp.sparseT = 0
	if nout == 0 {
		return gp.err(C.gogp_sparse_multi_set_outputs(gp.handle(), nil, 0, 0))
	}
	if nout < 0 || len(yt)%nout != 0 {
		return fmt.Errorf("len(yt)")
	}
	buf := yt
	if len(buf) == 0 {
		buf = make([]float64, 1)
	}
	if err := gp.err(C.gogp_sparse_multi_set_outputs(gp.handle(), dptr(buf), C.int64_t(len(yt)/nout), C.int32_t(nout))); err != nil {
		return err
	}
	gp.sparseT = nout
	return nil
}

// SparseMultiObserve computes the collapsed bound of every output column of
// SetSparseOutputs at x = log theta, on one pass over the data, and their sum
// in column order.
func (gp *GP) SparseMultiObserve(x []float64) (total float64, bounds []float64, err error) {
	gp.defaults()
	var t C.double
	buf := make([]float64, gp.sparseT+1)
	if err = gp.err(C.gogp_sparse_multi_observe(gp.handle(), dptr(x), C.int64_t(len(x)), &t, dptr(buf))); err != nil {
		return 0, nil, err
	}
	return float64(t), buf[:gp.sparseT], nil
}

// SparseMultiGradient computes the gradient of that sum with respect to the
// log-transformed hyperparameters, at the parameters of the last
// SparseMultiObserve.
func (gp *GP) SparseMultiGradient() ([]float64, error) {
	gp.defaults()
	g := make([]float64, len(gp.ThetaSimil)+len(gp.ThetaNoise))
	if err := gp.err(C.gogp_sparse_multi_gradient(gp.handle(), dptr(g), C.int64_t(len(g)))); err != nil {
		return nil, err
	}
	return g, nil
}

// SparseMultiGradientInducing computes SparseMultiGradient and, from the same
// pass over the data, the derivative of the sum in the inducing points of
// SetSparse (dU: row-major M x NDim).
func (gp *GP) SparseMultiGradientInducing() (grad, dU []float64, err error) {
	gp.defaults()
	if gp.sparseM < 1 {
		return nil, nil, fmt.Errorf("SparseMultiGradientInducing before SetSparse")
	}
	grad = make([]float64, len(gp.ThetaSimil)+len(gp.ThetaNoise))
	dU = make([]float64, gp.sparseM*gp.NDim)
	if err = gp.err(C.gogp_sparse_multi_gradient_inducing(gp.handle(), dptr(grad), C.int64_t(len(grad)), dptr(dU))); err != nil {
		return nil, nil, err
	}
	return grad, dU, nil
}

// SparseMultiProduce computes the predictive means of every output at the test
// points (row-major len(x) x nout) and the standard deviation they share
// (latent and unclamped, as SparseProduce).
func (gp *GP) SparseMultiProduce(x [][]float64) (mu, sigma []float64, err error) {
	gp.defaults()
	m := len(x)
	flat := make([]float64, m*gp.NDim)
	for i, row := range x {
		copy(flat[i*gp.NDim:], row)
	}
	buf, sigma := make([]float64, m*gp.sparseT+1), make([]float64, m)
	if err = gp.err(C.gogp_sparse_multi_produce(gp.handle(), dptr(flat), C.int64_t(m), dptr(buf), dptr(sigma))); err != nil {
		return nil, nil, err
	}
	return buf[:m*gp.sparseT], sigma, nil
}

// Sample draws len(xi)/len(x) joint samples at the test points from the
// caller's standard normals xi (row-major ns x m): samples[s*m+j] =
// mu[j] + (C xi[s])[j], C the lower Cholesky factor of the covariance +
// diagAdd I (no reference counterpart).
func (gp *GP) Sample(x [][]float64, xi []float64, diagAdd float64) (samples []float64, err error) {
	gp.defaults()
	m := len(x)
	ns := 0
	if m > 0 {
		ns = len(xi) / m
		if ns*m != len(xi) {
			return nil, fmt.Errorf("gogp: len(xi) = %d is no multiple of %d test points", len(xi), m)
		}
	}
	flat := make([]float64, m*gp.NDim)
	for i, row := range x {
		copy(flat[i*gp.NDim:], row)
	}
	mu := make([]float64, m)
	samples = make([]float64, ns*m)
	if err = gp.err(C.gogp_produce_samples(gp.handle(), dptr(flat), C.int64_t(m), dptr(xi), C.int64_t(ns), C.double(diagAdd), dptr(mu), dptr(samples))); err != nil {
		return nil, err
	}
	return samples, nil
}

// Observe computes the log marginal likelihood of log-transformed
// hyperparameters [, inputs, outputs] (gp/gp.go:374-413).  Panics where the
// reference panics.
func (gp *GP) Observe(x []float64) float64 {
	gp.defaults()
	P := len(gp.ThetaSimil) + len(gp.ThetaNoise)
	var lml C.double
	var rc C.int
	if len(x) == P {
		if err := gp.pushData(); err != nil {
			panic(err)
		}
		gp.withObs = false
		rc = C.gogp_observe(gp.handle(), dptr(x), C.int64_t(len(x)), &lml)
	} else {
		rest := len(x) - P
		if rest < 0 || rest%(gp.NDim+1) != 0 {
			panic("len(x)") // gp/gp.go:398-400
		}
		gp.withObs = true
		rc = C.gogp_observe_full(gp.handle(), dptr(x), C.int64_t(len(x)), &lml)
		n := rest / (gp.NDim + 1) // gp/gp.go:391-396: X, Y re-sliced from x
		gp.X = make([][]float64, n)
		for i := range gp.X {
			gp.X[i] = x[P+i*gp.NDim : P+(i+1)*gp.NDim]
		}
		gp.Y = x[P+n*gp.NDim:]
		// the device holds exactly these data now (gogp_observe_full replaced them), unless the
		// call failed half-way
		gp.dirty, gp.upN = rc != C.GOGP_OK, n
		if n > 0 {
			gp.upX, gp.upY = &gp.X[0], &gp.Y[0]
		}
	}
	if err := gp.err(rc); err != nil {
		panic(err) // gp/gp.go:402-405 (also gonum's Condition error: GOGP_ECOND)
	}
	if err := gp.fetchState(); err != nil { // Alpha is part of the documented state (gp/gp.go:255-257)
		panic(err)
	}
	for i := range gp.ThetaSimil { // gp/gp.go:384-385
		gp.ThetaSimil[i] = math.Exp(x[i])
	}
	for i := range gp.ThetaNoise {
		gp.ThetaNoise[i] = math.Exp(x[len(gp.ThetaSimil)+i])
	}
	gp.lastLen = len(x)
	return float64(lml)
}

// ObserveGradientCandidates evaluates k candidate log-theta vectors (hyperparameters-only form)
// on the GP's data in ONE launch sequence and returns what Observe + Gradient would return for
// each; the GP's own state is not touched.  status[c] is C.GOGP_ENOTPD where the matrix of
// candidate c is not positive definite (lml NaN, gradient zeros).  This is the device-side
// form of optimize.Settings.Concurrent (tutorial/tutorial.go:30,141): one GP instead of NTASKS.
func (gp *GP) ObserveGradientCandidates(xs [][]float64) (lml []float64, grad [][]float64, status []int) {
	k, p := len(xs), len(gp.ThetaSimil)+len(gp.ThetaNoise)
	flat := make([]float64, k*p)
	for c, x := range xs {
		if len(x) != p {
			panic("len(x)") // gp/gp.go:398-400
		}
		copy(flat[c*p:], x)
	}
	if err := gp.pushData(); err != nil {
		panic(err)
	}
	lml = make([]float64, k)
	gflat := make([]float64, k*p)
	st := make([]C.int, k)
	rc := C.gogp_observe_gradient_candidates(gp.handle(), C.int(k), dptr(flat), C.int64_t(p),
		dptr(lml), dptr(gflat), &st[0])
	if rc != C.GOGP_OK && rc != C.GOGP_ENOTPD && rc != C.GOGP_ECOND {
		panic(gp.err(rc))
	}
	grad, status = make([][]float64, k), make([]int, k)
	for c := range grad {
		grad[c] = gflat[c*p : (c+1)*p]
		status[c] = int(st[c])
	}
	return lml, grad, status
}

// SetOption sets a schedule / precision option of the device path (gogp_set_option; no reference
// counterpart).  "gradient_precision" = 32 keeps Observe's LML, Alpha and Produce in fp64 and runs
// what only Gradient needs (the triangular inverse and K^-1) on the fp32 matrix cores: the gradient
// stays within ~1e-8 of the fp64 one (the reference checks its own to 1e-4, gp/gp_test.go:170,248)
// at 19 instead of 14 evaluations per second at N = 16384.  Only for kernels of ONE term with an output
// scale: for a sum of terms the library refuses the option (an error) rather than return scale components
// read off the float K^-1 (1.9e-4 measured).
func (gp *GP) SetOption(name string, value int64) error {
	cn := C.CString(name)
	defer C.free(unsafe.Pointer(cn))
	return gp.err(C.gogp_set_option(gp.handle(), cn, C.int64_t(value)))
}

// Gradient computes the gradient of the log-likelihood (gp/gp.go:418-499).
func (gp *GP) Gradient() []float64 {
	grad := make([]float64, gp.lastLen)
	if err := gp.err(C.gogp_gradient(gp.handle(), dptr(grad), C.int64_t(len(grad)))); err != nil {
		panic(err)
	}
	return grad
}
