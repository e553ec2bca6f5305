// pitch.hip -- Audio::get_local_wavelength(s) and what rests on them (Audio/AudioInformation.cpp:18-75, 138-265; DSPUtility.cpp:37-147): the
// YIN pitch tracker.  DESIGN.md section 4.21.
//
// Per analysis window of n samples, h = n / 2:
//   d[tau]  = sum_{i<h} ( x[i] - x[i+tau] )^2, tau < h                       (compute_d, :18-57; the reference gets it from two fp32 FFTs)
//   d'[0]   = 1, d'[tau] = float( double( d[tau] ) * ( tau / sum_{1..tau} d ) ), 1 where the sum is 0      (compute_d_prime, :59-75)
//   valleys of d' (find_valleys with its defaults), the three-step selection (:149-165) -> one wavelength in frames, or 0
// The windows are independent, so a block takes one window:
//   yin_dprime_block   the n samples staged in LDS; a thread owns FOUR CONSECUTIVE lags and walks i four at a time, so 16 terms cost
//                      two 16-byte LDS reads (x[i..i+3], a broadcast, and x[i+tau0+4 .. +7]; the four samples before them are the step before's).
//                      A term is an fp32 difference and an explicit fmaf (the library is built with -ffp-contract=off); 32 terms
//                      are chained in fp32, the chunks are added in fp64: every term is >= 0, nothing cancels.  d is rounded to fp32 --
//                      the reference's d is fp32 --, then summed over tau in fp64 (per-thread runs, a 256-wide scan of their totals,
//                      the runs again) and normalised
//   yin_pick_block     a d' row in LDS -> the wavelength.  fp32, the reference's operations in its order; integer-valued reductions
//                      otherwise, so the answer is a function of the row's bits alone.  The reference walks from every point to the
//                      first differing value on either side, O( h ) per point on a flat row; here only the LEFTMOST point of a run of
//                      equal values walks, once, over its run.  Valleys come out ordered by index, which is the reference's order by
//                      x: interpolated x lies within half a frame of its point, a plateau's x inside the plateau.
// k_yin_dprime and k_yin_pick wrap one each, k_yin_fused both with d' never leaving LDS; the same code on the same values, so fused
// and split agree bit for bit.  A row with a NaN or an infinity gives 0 (documented in flanhip.h).
#include "flanhip_internal.h"

#include <cfloat>
#include <climits>

namespace flanhip {

namespace {

constexpr int YIN_THREADS = 256;
constexpr int YIN_CHUNK = 32;                                  // i-steps chained in fp32 before they are added in fp64; a multiple of 4
constexpr int YIN_PAD = 8;                                     // floats behind the samples that the 16-byte reads of lags >= h may touch
constexpr int64_t YIN_MAX_WINDOW = 16384;                      // n: the samples, d' and the scratch of a block in LDS
constexpr int64_t YIN_MAX_H = YIN_MAX_WINDOW / 2;
constexpr size_t YIN_SCRATCH_BYTES = sizeof( double ) * YIN_THREADS;

// The dynamic LDS of a block, every part a multiple of 16 bytes: the samples (n + YIN_PAD floats; the pick's x and y rows, 2 h floats,
// lie over them), the row d / d' (h floats), the scratch of the scan and of the reductions
__host__ __device__ constexpr int yin_pad4( int v ) { return ( v + 3 ) & ~3; }
__host__ __device__ constexpr int yin_samples_floats( int n ) { return yin_pad4( n + YIN_PAD ); }
size_t yin_lds_bytes( int n, int h ) { return sizeof( float ) * size_t( yin_samples_floats( n ) + yin_pad4( h ) ) + YIN_SCRATCH_BYTES; }

struct YinLds { float * samples; float * row; double * scratch; };
__device__ __forceinline__ YinLds yin_lds( char * base, int n, int h )
	{
	YinLds l;
	l.samples = reinterpret_cast<float*>( base );
	l.row = l.samples + yin_samples_floats( n );
	l.scratch = reinterpret_cast<double*>( l.row + yin_pad4( h ) );
	return l;
	}

// ---- d and d' ----------------------------------------------------------------------------------------------------------------------
// x (global): the window's n samples.  Leaves d' in row[0..h); samples is free afterwards.  All threads of the block call it
__device__ void yin_dprime_block( const float * __restrict__ x, int n, int h, const YinLds & l )
	{
	float * sx = l.samples;
	float * sd = l.row;
	const int tid = threadIdx.x;
	for( int i = tid; i < yin_samples_floats( n ); i += YIN_THREADS ) sx[i] = i < n ? x[i] : 0.0f;
	__syncthreads();

	const int h4 = h & ~3;
	for( int tau0 = 4 * tid; tau0 < h; tau0 += 4 * YIN_THREADS )
		{
		const float * xs = sx + tau0;
		double D[4] = { 0.0, 0.0, 0.0, 0.0 };
		float4 b = *reinterpret_cast<const float4*>( xs );                 // x[i + tau0 .. + 3]: the upper half of one step is the lower half of the next
		for( int i0 = 0; i0 < h4; i0 += YIN_CHUNK )
			{
			float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
			const int i1 = i0 + YIN_CHUNK < h4 ? i0 + YIN_CHUNK : h4;
			for( int i = i0; i < i1; i += 4 )
				{
				const float4 a = *reinterpret_cast<const float4*>( sx + i );
				const float4 c = *reinterpret_cast<const float4*>( xs + i + 4 );
				const float av[4] = { a.x, a.y, a.z, a.w };
				const float w[8] = { b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
				#pragma unroll
				for( int j = 0; j < 4; ++j )
					{
					#pragma unroll
					for( int k = 0; k < 4; ++k )
						{
						const float e = av[j] - w[j + k];
						acc[k] = fmaf( e, e, acc[k] );
						}
					}
				b = c;
				}
			#pragma unroll
			for( int k = 0; k < 4; ++k ) D[k] += double( acc[k] );
			}
		if( h4 < h )
			{
			float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
			for( int i = h4; i < h; ++i )
				{
				const float a = sx[i];
				#pragma unroll
				for( int k = 0; k < 4; ++k )
					{
					const float e = a - xs[i + k];
					acc[k] = fmaf( e, e, acc[k] );
					}
				}
			#pragma unroll
			for( int k = 0; k < 4; ++k ) D[k] += double( acc[k] );
			}
		#pragma unroll
		for( int k = 0; k < 4; ++k ) if( tau0 + k < h ) sd[tau0 + k] = float( D[k] );
		}
	__syncthreads();

	// :64-72: the running sum over tau >= 1 in double; a thread takes a run of consecutive lags
	const int run = ( h + YIN_THREADS - 1 ) / YIN_THREADS;
	const int t0 = tid * run < h ? tid * run : h, t1 = t0 + run < h ? t0 + run : h;
	double total = 0.0;
	for( int tau = t0 > 1 ? t0 : 1; tau < t1; ++tau ) total += double( sd[tau] );
	double * part = l.scratch;
	part[tid] = total;
	__syncthreads();
	for( int step = 1; step < YIN_THREADS; step <<= 1 )
		{
		const double below = tid >= step ? part[tid - step] : 0.0;
		__syncthreads();
		part[tid] += below;
		__syncthreads();
		}
	double sum = tid > 0 ? part[tid - 1] : 0.0;
	for( int tau = t0; tau < t1; ++tau )
		{
		if( tau == 0 ) { sd[0] = 1.0f; continue; }
		const double d = double( sd[tau] );
		sum += d;
		sd[tau] = sum == 0.0 ? 1.0f : float( d * ( double( tau ) / sum ) );
		}
	__syncthreads();
	}

// ---- the pick ----------------------------------------------------------------------------------------------------------------------
// the smaller y, the smaller index among equal y, of the block's ( y, index ) pairs; ( +inf, INT_MAX ): none.  All threads get the result
__device__ void yin_block_min( float & y, int & index, float * sy, int * si )
	{
	const int tid = threadIdx.x;
	sy[tid] = y; si[tid] = index;
	__syncthreads();
	for( int step = YIN_THREADS / 2; step > 0; step >>= 1 )
		{
		if( tid < step )
			{
			const float y2 = sy[tid + step];
			const int i2 = si[tid + step];
			if( y2 < sy[tid] || ( y2 == sy[tid] && i2 < si[tid] ) ) { sy[tid] = y2; si[tid] = i2; }
			}
		__syncthreads();
		}
	y = sy[0]; index = si[0];
	__syncthreads();
	}

// DSPUtility.cpp:37-43 on -d' with y negated back (:139-140), operation by operation
__device__ __forceinline__ void yin_parabola( float d0, float d1, float d2, int x1, float & X, float & Y )
	{
	const float y0 = -d0, y1 = -d1, y2 = -d2;
	const float delta_x = 0.5f * ( y0 - y2 ) / ( y0 - 2.0f * y1 + y2 );
	X = float( x1 ) + delta_x;
	Y = -( y1 - 0.25f * ( y0 - y2 ) * delta_x );
	}

// row: d' in LDS, h >= 3.  vx, vy: h floats each of LDS scratch.  The wavelength, the same value in every thread
__device__ float yin_pick_block( const float * row, int h, float absolute_cutoff, float minimum_wavelength, float * vx, float * vy, double * scratch )
	{
	const int tid = threadIdx.x;
	float * ry = reinterpret_cast<float*>( scratch );
	int * ri = reinterpret_cast<int*>( scratch ) + YIN_THREADS;

	// a NaN or an infinity anywhere in the row: no wavelength
	bool bad = false;
	for( int i = tid; i < h; i += YIN_THREADS ) bad = bad || !( fabsf( row[i] ) <= FLT_MAX );
	if( tid == 0 ) ri[0] = 0;
	__syncthreads();
	if( bad ) ri[0] = 1;
	__syncthreads();
	const bool any_bad = ri[0] != 0;
	__syncthreads();
	if( any_bad ) return 0.0f;

	// the valleys (DSPUtility.cpp:65-118), kept at the leftmost point of their run: vx < 0 marks a point that keeps none
	for( int tau = 1 + tid; tau <= h - 2; tau += YIN_THREADS )
		{
		const float v = row[tau];
		float X = -1.0f, Y = 0.0f;
		if( row[tau - 1] > v )                                            // the run begins here and the left side rises
			{
			int right = tau + 1;
			while( right < h && row[right] == v ) ++right;
			if( right < h && row[right] > v )                             // not the edge, and the right side rises too
				{
				const int left = tau - 1;
				if( right - left > 2 ) { X = float( ( right + left ) * 0.5 ); Y = v; }        // :93-103: the plateau's middle, the plain value
				else yin_parabola( row[tau - 1], v, row[tau + 1], tau, X, Y );
				}
			}
		vx[tau] = X; vy[tau] = Y;
		}
	__syncthreads();

	// AudioInformation.cpp:149-153: among the valleys with minimum_wavelength < x, the first lowest y
	float low_y = INFINITY;
	int low_i = INT_MAX;
	for( int tau = 1 + tid; tau <= h - 2; tau += YIN_THREADS )
		if( vx[tau] >= 0.0f && minimum_wavelength < vx[tau] && vy[tau] < low_y ) { low_y = vy[tau]; low_i = tau; }
	yin_block_min( low_y, low_i, ry, ri );
	if( low_i == INT_MAX ) return 0.0f;                                   // :150

	// :159-162: the first of them with y < lowest.y * 2
	const float limit = low_y * 2.0f;
	float any_y = INFINITY;
	int best_i = INT_MAX;
	for( int tau = 1 + tid; tau <= h - 2 && best_i == INT_MAX; tau += YIN_THREADS )
		if( vx[tau] >= 0.0f && minimum_wavelength < vx[tau] && vy[tau] < limit ) { any_y = 0.0f; best_i = tau; }
	yin_block_min( any_y, best_i, ry, ri );
	const float best_x = best_i == INT_MAX ? 0.0f : vx[best_i], best_y = best_i == INT_MAX ? 0.0f : vy[best_i];   // vec2(): ( 0, 0 )
	return best_y < absolute_cutoff ? best_x : 0.0f;                      // :164-165
	}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------
// one block per window: window w begins at frame first + w * hop of x
__global__ __launch_bounds__( YIN_THREADS ) void k_yin_dprime( const float * __restrict__ x, int64_t first, int64_t hop, int n, int h, float * __restrict__ dprime )
	{
	extern __shared__ __attribute__( ( aligned( 16 ) ) ) char s_yin[];
	const YinLds l = yin_lds( s_yin, n, h );
	yin_dprime_block( x + first + int64_t( blockIdx.x ) * hop, n, h, l );
	float * out = dprime + int64_t( blockIdx.x ) * h;
	for( int i = threadIdx.x; i < h; i += YIN_THREADS ) out[i] = l.row[i];
	}

__global__ __launch_bounds__( YIN_THREADS ) void k_yin_pick( const float * __restrict__ dprime, int h, float absolute_cutoff, float minimum_wavelength, float * __restrict__ out )
	{
	extern __shared__ __attribute__( ( aligned( 16 ) ) ) char s_yin[];
	const YinLds l = yin_lds( s_yin, 2 * h, h );
	const float * in = dprime + int64_t( blockIdx.x ) * h;
	for( int i = threadIdx.x; i < h; i += YIN_THREADS ) l.row[i] = in[i];
	__syncthreads();
	const float w = yin_pick_block( l.row, h, absolute_cutoff, minimum_wavelength, l.samples, l.samples + h, l.scratch );
	if( threadIdx.x == 0 ) out[blockIdx.x] = w;
	}

__global__ __launch_bounds__( YIN_THREADS ) void k_yin_fused( const float * __restrict__ x, int64_t first, int64_t hop, int n, int h, float absolute_cutoff,
	float minimum_wavelength, float * __restrict__ out )
	{
	extern __shared__ __attribute__( ( aligned( 16 ) ) ) char s_yin[];
	const YinLds l = yin_lds( s_yin, n, h );
	yin_dprime_block( x + first + int64_t( blockIdx.x ) * hop, n, h, l );
	const float w = yin_pick_block( l.row, h, absolute_cutoff, minimum_wavelength, l.samples, l.samples + h, l.scratch );
	if( threadIdx.x == 0 ) out[blockIdx.x] = w;
	}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
struct YinShape { int64_t count = 0; int n = 0, h = 0; };

// :180-183: the windows at start, start + hop, ... while frame + window < end; -1 for arguments every form refuses
int64_t yin_count( int64_t num_frames, int64_t start, int64_t end, int64_t window, int64_t hop )
	{
	if( end == -1 ) end = num_frames;
	if( num_frames < 0 || hop < 1 || start < 0 || end < 0 || end > num_frames || window < 1 ) return -1;
	if( window >= end || start >= end - window ) return 0;                // frame < end - window
	return ( end - window - start - 1 ) / hop + 1;
	}

// what every form refuses before any device call
int yin_check( int64_t num_frames, int64_t start, int64_t end, int64_t window, int64_t hop, YinShape * s )
	{
	FLANHIP_REQUIRE( num_frames >= 0 && window >= 1, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( hop >= 1, FLANHIP_ERR_INVALID_ARG, "hop below 1" );
	FLANHIP_REQUIRE( start >= 0 && ( end == -1 || ( end >= 0 && end <= num_frames ) ), FLANHIP_ERR_INVALID_ARG, "range outside the signal" );
	FLANHIP_REQUIRE( window <= YIN_MAX_WINDOW, FLANHIP_ERR_UNSUPPORTED, "window above 16384" );
	s->count = yin_count( num_frames, start, end, window, hop );
	s->n = int( window ); s->h = int( window / 2 );
	return FLANHIP_OK;
	}

int launch_yin_dprime( const float * d_x, int64_t start, int64_t hop, const YinShape & sh, float * d_dprime, hipStream_t s )
	{
	return launch_kernel( "launch_yin_dprime", k_yin_dprime, sh.count, YIN_THREADS, yin_lds_bytes( sh.n, sh.h ), s, d_x, start, hop, sh.n, sh.h, d_dprime );
	}

int launch_yin_pick( const float * d_dprime, int64_t count, int h, float absolute_cutoff, int64_t minimum_wavelength, float * d_out, hipStream_t s )
	{
	return launch_kernel( "launch_yin_pick", k_yin_pick, count, YIN_THREADS, yin_lds_bytes( 2 * h, h ), s, d_dprime, h, absolute_cutoff,
		float( minimum_wavelength ), d_out );
	}

// the raw wavelengths of sh.count windows; h < 3 has no interior point: zeros, no launch
int launch_yin( const float * d_x, int64_t start, int64_t hop, const YinShape & sh, float absolute_cutoff, int64_t minimum_wavelength, float * d_out, hipStream_t s )
	{
	if( sh.count == 0 ) return FLANHIP_OK;
	if( sh.h < 3 ) { FLANHIP_CHECK( hipMemsetAsync( d_out, 0, sizeof( float ) * size_t( sh.count ), s ) ); return FLANHIP_OK; }
	return launch_kernel( "launch_yin", k_yin_fused, sh.count, YIN_THREADS, yin_lds_bytes( sh.n, sh.h ), s, d_x, start, hop, sh.n, sh.h, absolute_cutoff,
		float( minimum_wavelength ), d_out );
	}

// ---- host-only parts ---------------------------------------------------------------------------------------------------------------
// AudioInformation.cpp:190-226 as written
void yin_continuity( float * out, int64_t size, float sample_rate, int64_t hop_size )
	{
	const float minimum_note_length = 0.1f;                               // :193
	const int minimum_num_hops = int( ( minimum_note_length * sample_rate ) / float( hop_size ) );   // :194, time_to_frame( t ) = t * sr (AudioBuffer.cpp:406-409)
	std::vector<int64_t> sus_hops;
	for( int64_t i = 0; i < size - 1; ++i )                               // :198-204
		{
		if( out[i] == 0 ) continue;
		const float r = out[i + 1] / out[i];
		if( 1.95 < r && r < 2.05 ) sus_hops.push_back( i + 1 );          // double literals
		}
	for( int64_t hop : sus_hops )                                         // :207-226
		{
		int sus_length = 0;
		do
			{
			const int64_t global_hop = hop + sus_length;
			if( global_hop >= size ) break;
			if( out[global_hop] == 0 ) continue;                          // to the loop's condition
			const float r = out[global_hop] / out[hop];
			if( r < .95f || r > 1.05f ) break;
			} while( ++sus_length <= minimum_num_hops );
		if( sus_length > minimum_num_hops ) break;                        // leaves the loop over the suspicious hops
		for( int64_t i = hop; i < hop + sus_length; ++i ) out[i] /= 2.0f;
		}
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

int64_t flanhip_audio_local_wavelengths_count( int64_t num_frames, int64_t start, int64_t end, int64_t window, int64_t hop )
	{
	return yin_count( num_frames, start, end, window, hop );
	}

size_t flanhip_audio_local_wavelengths_workspace_bytes( int64_t num_frames, int64_t start, int64_t end, int64_t window, int64_t hop )
	{
	if( yin_count( num_frames, start, end, window, hop ) < 0 || window > YIN_MAX_WINDOW ) return 0;
	return 16;
	}

int flanhip_audio_yin_dprime_dev( const float * d_x, int64_t num_frames, int64_t start, int64_t end, int64_t window, int64_t hop, float * d_dprime, void * stream )
	{
	FLANHIP_REQUIRE( d_x && d_dprime, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	YinShape sh;
	if( int rc = yin_check( num_frames, start, end, window, hop, &sh ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( sh.count == 0 || sh.h == 0 ) return FLANHIP_OK;
	return launch_yin_dprime( d_x, start, hop, sh, d_dprime, (hipStream_t) stream );
	}

int flanhip_audio_yin_pick_dev( const float * d_dprime, int64_t count, int64_t h, float absolute_cutoff, int64_t minimum_wavelength, float * d_out, void * stream )
	{
	FLANHIP_REQUIRE( d_dprime && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( count >= 0 && h >= 0, FLANHIP_ERR_INVALID_ARG, "negative size" );
	FLANHIP_REQUIRE( h <= YIN_MAX_H, FLANHIP_ERR_UNSUPPORTED, "row above 8192" );
	if( int rc = require_device() ) return rc;
	if( count == 0 ) return FLANHIP_OK;
	if( h < 3 ) { FLANHIP_CHECK( hipMemsetAsync( d_out, 0, sizeof( float ) * size_t( count ), (hipStream_t) stream ) ); return FLANHIP_OK; }
	return launch_yin_pick( d_dprime, count, int( h ), absolute_cutoff, minimum_wavelength, d_out, (hipStream_t) stream );
	}

int flanhip_audio_local_wavelengths_dev( const float * d_x, int64_t num_frames, int64_t start, int64_t end, int64_t window, int64_t hop,
	float absolute_cutoff, int64_t minimum_wavelength, float * d_out, void * d_workspace, void * stream )
	{
	FLANHIP_REQUIRE( d_x && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	YinShape sh;
	if( int rc = yin_check( num_frames, start, end, window, hop, &sh ) ) return rc;
	if( int rc = require_device() ) return rc;
	return launch_yin( d_x, start, hop, sh, absolute_cutoff, minimum_wavelength, d_out, (hipStream_t) stream );
	}

int flanhip_audio_local_wavelength_dev( const float * d_window, int64_t window, float absolute_cutoff, int64_t minimum_wavelength, float * d_out, void * stream )
	{
	FLANHIP_REQUIRE( d_window && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( window >= 1, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( window <= YIN_MAX_WINDOW, FLANHIP_ERR_UNSUPPORTED, "window above 16384" );
	if( int rc = require_device() ) return rc;
	YinShape sh;
	sh.count = 1; sh.n = int( window ); sh.h = int( window / 2 );
	return launch_yin( d_window, 0, 1, sh, absolute_cutoff, minimum_wavelength, d_out, (hipStream_t) stream );
	}

int flanhip_audio_local_wavelengths( const float * x, int64_t num_frames, float sample_rate, int64_t start, int64_t end, int64_t window, int64_t hop,
	float absolute_cutoff, int64_t minimum_wavelength, float * out, volatile int * cancel )
	{
	FLANHIP_REQUIRE( x && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	YinShape sh;
	if( int rc = yin_check( num_frames, start, end, window, hop, &sh ) ) return rc;
	if( sh.count == 0 ) return FLANHIP_OK;
	if( sh.h < 3 ) { std::fill( out, out + sh.count, 0.0f ); return FLANHIP_OK; }      // no interior point: no device call, and halving zeros changes nothing
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	// only what the windows read goes up: frames [start, last window's end)
	const int64_t span = ( sh.count - 1 ) * hop + window;
	HostCall call( cancel );
	const float * d_x = nullptr;
	float * d_out = nullptr;
	if( int rc = call.in( x + start, sizeof( float ) * size_t( span ), &d_x ) ) return rc;
	if( int rc = call.out( out, sizeof( float ) * size_t( sh.count ), &d_out ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_yin( d_x, 0, hop, sh, absolute_cutoff, minimum_wavelength, d_out, nullptr ) ) return rc;
	if( int rc = call.finish() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	yin_continuity( out, sh.count, sample_rate, hop );
	return FLANHIP_OK;
	}

int flanhip_wavelength_continuity( float * w, int64_t count, float sample_rate, int64_t hop )
	{
	FLANHIP_REQUIRE( w || count == 0, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( count >= 0, FLANHIP_ERR_INVALID_ARG, "negative size" );
	FLANHIP_REQUIRE( hop >= 1, FLANHIP_ERR_INVALID_ARG, "hop below 1" );
	if( count > 0 ) yin_continuity( w, count, sample_rate, hop );
	return FLANHIP_OK;
	}

// :245-265 with mean_and_sd (DSPUtility.cpp:159-185): fp32, in order
int flanhip_average_wavelength( const float * locals, int64_t count, float min_active_ratio, float max_length_sigma, float * out )
	{
	FLANHIP_REQUIRE( out && ( locals || count == 0 ), FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( count >= 0, FLANHIP_ERR_INVALID_ARG, "negative size" );
	const size_t size = size_t( count );
	const int num_valids = int( count - std::count( locals, locals + count, -1.0f ) );
	if( num_valids <= min_active_ratio * size ) { *out = -1.0f; return FLANHIP_OK; }       // :257
	int n = 0;
	float sum = 0;
	for( size_t i = 0; i < size; ++i ) if( locals[i] != 0 ) { sum += locals[i]; ++n; }     // :259: zeros go, -1 stays
	float mean = 0, sd = 0;
	if( n > 0 )
		{
		mean = sum / n;
		float diff_sum = 0;
		for( size_t i = 0; i < size; ++i ) if( locals[i] != 0 ) { const float d = locals[i] - mean; diff_sum += d * d; }
		sd = std::sqrt( diff_sum / n );
		}
	*out = max_length_sigma != -1 && sd > max_length_sigma ? -1.0f : mean;                 // :262-264
	return FLANHIP_OK;
	}

} // extern "C"
