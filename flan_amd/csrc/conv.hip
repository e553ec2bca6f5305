// conv.hip -- Audio::convolve (Audio/AudioCombination.cpp:299-352): linear convolution of every channel with an impulse response,
// by uniformly partitioned overlap-save (UPOLS).  DESIGN.md section 4.12.
//
// The reference takes one real FFT of size D = 2 pow2( max( n, m ) ) per channel.  Here both signals are cut into partitions of P
// samples and every transform has 2P real points (P complex points plus the real split / merge, as in fft_device.h):
//   H_i = rfft( h[iP, (i+1)P) zero-padded to 2P )              i < K = ceil( m / P )       k_conv_spectra, once per IR channel used
//   X_j = rfft( x[(j-1)P, (j+1)P) ), zeros outside [0, n)      j < J = ceil( (n+m) / P )   k_conv_spectra
//   Y_j = sum_{i < min(j+1, K)} X_{j-i} H_i                    per bin                     k_conv_delay (a frequency-domain delay line)
//   y[jP, (j+1)P) = last P samples of irfft( Y_j )                                         k_conv_inverse (+ the max |y| of normalize)
// and, with normalize, out *= 1.0f / max |y| over the reference's frame range (k_conv_scale; the reciprocal is taken on the device).
// Every sum runs in a fixed order and the max is an atomic max on the bits of non-negative floats, so two runs agree bit for bit.
#include "flanhip_internal.h"
#include "fft_device.h"

#include <algorithm>

namespace flanhip {

namespace {

thread_local int t_conv_partition = 0;    // flanhip_convolve_debug_partition: P forced for the calling thread (0: the library's choice)

constexpr int CONV_TEAM = 256;            // threads per transform (k_conv_spectra / k_conv_inverse)
constexpr int CONV_T = 16;                // output partitions per thread of the delay line (its accumulators)
constexpr int CONV_DELAY_THREADS = 256;
constexpr int CONV_MIN_P = 512, CONV_MAX_P = 4096;     // the library's choices (fft_device.h's fft_forward serves up to 2^12 complex points)
constexpr int CONV_MIN_FORCED_P = 128;                 // smaller partitions only when forced (tests: K = 32 where P = 4096 gives K = 1)
constexpr int CONV_MAX_K = 32;
// normalize: the inverse blocks' maxima go to 64 words 128 bytes apart (block b to word b mod 64), since tens of thousands of atomics on
// ONE word serialise (8 ch x 60 s at P = 1024: the inverse pass took 274 us with one word); k_conv_scale reduces the 64
constexpr int CONV_MAX_SLOTS = 64, CONV_SLOT_STRIDE = 32;
constexpr size_t CONV_MAX_BYTES = sizeof( unsigned ) * CONV_MAX_SLOTS * CONV_SLOT_STRIDE;

struct ConvShape
	{
	int P = 0, log2P = 0;
	int64_t K = 0, J = 0, Jx = 0;          // IR partitions, output partitions, input spectra that are not all zeros
	int64_t ir_used = 0;                   // IR channels an output channel reads (channel c uses c % ir_channels)
	size_t x_off = 0, h_off = 0, y_off = 0, word_off = 0, total = 0;
	};

// smallest P with K <= 32, capped at the largest supported; or the calling thread's forced P (0 if that is not a supported size)
int conv_partition( int64_t m )
	{
	if( const int forced = t_conv_partition )
		return ( is_pow2( forced ) && forced >= CONV_MIN_FORCED_P && forced <= CONV_MAX_P ) ? forced : 0;
	int P = CONV_MIN_P;
	while( P < CONV_MAX_P && ( m + P - 1 ) / P > CONV_MAX_K ) P *= 2;
	return P;
	}

bool conv_sizes_ok( int64_t ch, int64_t n, int64_t irch, int64_t m )
	{
	return ch > 0 && n > 0 && irch > 0 && m > 0 && n <= ( int64_t( 1 ) << 40 ) && m <= ( int64_t( 1 ) << 40 ) && ch <= ( 1 << 20 ) && irch <= ( 1 << 20 );
	}

bool conv_shape( int64_t ch, int64_t n, int64_t irch, int64_t m, ConvShape * s )
	{
	if( !conv_sizes_ok( ch, n, irch, m ) ) return false;
	s->P = conv_partition( m );
	if( !s->P ) return false;
	s->log2P = ilog2( s->P );
	const int64_t P = s->P, B = P + 1;
	s->K = ( m + P - 1 ) / P;
	s->J = ( n + m + P - 1 ) / P;
	s->Jx = std::min( s->J, ( n + P - 1 ) / P + 1 );
	s->ir_used = std::min( ch, irch );
	const size_t row = sizeof( cf ) * size_t( B );
	s->x_off = 0;
	s->h_off = s->x_off + row * size_t( ch ) * size_t( s->J );
	s->y_off = s->h_off + row * size_t( s->ir_used ) * size_t( s->K );
	s->word_off = s->y_off + row * size_t( ch ) * size_t( s->J );
	s->total = s->word_off + CONV_MAX_BYTES;
	// launch limits: every grid below stays under 2^24 blocks (2^32 work-items)
	const int64_t delay_blocks = ch * ( ( s->J + CONV_T - 1 ) / CONV_T ) * ( ( B + CONV_DELAY_THREADS - 1 ) / CONV_DELAY_THREADS );
	return ch * s->J < ( int64_t( 1 ) << 24 ) && s->ir_used * s->K < ( int64_t( 1 ) << 24 ) && delay_blocks < ( int64_t( 1 ) << 24 );
	}

// rfft of 2P = 2C real points per block: src rows of `len` samples; block b -> row b / parts, partition j = b % parts; the 2C samples
// start at j C - shift and only the first `lim` of them are taken (the rest are zeros), as are samples outside [0, len).
// dst[( row dst_parts + j ) (C+1) + k], k = 0 .. C.
template<int LOG2C>
__global__ __launch_bounds__( CONV_TEAM ) void k_conv_spectra( const float * __restrict__ src, int64_t len, int64_t parts, int64_t dst_parts,
	int64_t shift, int lim, cf * __restrict__ dst, const cf * __restrict__ g_tw, const cf * __restrict__ g_tw2 )
	{
	constexpr int C = 1 << LOG2C;
	__shared__ cf s_mem[padded_len( C ) + C];
	cf * buf = s_mem;
	cf * tw = s_mem + padded_len( C );
	const int lane = threadIdx.x;
	const int64_t row = int64_t( blockIdx.x ) / parts, j = int64_t( blockIdx.x ) - row * parts;
	const float * x = src + row * len;
	const int64_t start = j * C - shift;
	for( int i = lane; i < C; i += CONV_TEAM )
		{
		tw[i] = g_tw[i];
		const int s0 = 2 * i, s1 = 2 * i + 1;
		const int64_t a0 = start + s0, a1 = start + s1;
		const float v0 = ( s0 < lim && a0 >= 0 && a0 < len ) ? x[a0] : 0.0f;
		const float v1 = ( s1 < lim && a1 >= 0 && a1 < len ) ? x[a1] : 0.0f;
		buf[PAD( i )] = mk( v0, v1 );
		}
	__syncthreads();
	fft_forward<LOG2C, CONV_TEAM>( buf, tw, lane );
	// split the half-size transform into the real transform's bins (as k_analyze does, pv_kernels.h)
	cf * out = dst + ( row * dst_parts + j ) * ( C + 1 );
	const cf z0 = buf[PAD( 0 )];
	for( int k = lane; k < C; k += CONV_TEAM )
		{
		const cf zk = buf[PAD( k )];
		const cf zm = buf[PAD( ( C - k ) & ( C - 1 ) )];
		const float ax = 0.5f * ( zk.x + zm.x ), ay = 0.5f * ( zk.y - zm.y );
		const float dx = zk.x - zm.x, dy = zk.y + zm.y;
		const cf w2v = g_tw2[k];
		const float c = w2v.x, s = w2v.y;
		float re = ax + 0.5f * __builtin_fmaf( c, dy, s * dx );
		float im = ay - 0.5f * __builtin_fmaf( c, dx, -( s * dy ) );
		if( k == 0 ) { re = z0.x + z0.y; im = 0.0f; }
		out[k] = mk( re, im );
		}
	if( lane == 0 ) out[C] = mk( z0.x - z0.y, 0.0f );
	}

// The delay line: one thread per (channel, bin, tile of T consecutive output partitions j0 .. j0+T-1), T accumulators in registers.
// Step i loads H_i and one new X (X_{j0-i-1}, which every later step needs); the T spectra in flight sit in a ring indexed by the
// partition number mod T, so with the inner loop unrolled every index is a constant.  Lanes are consecutive bins of one (channel, tile).
template<int T>
__global__ __launch_bounds__( CONV_DELAY_THREADS ) void k_conv_delay( const cf * __restrict__ X, const cf * __restrict__ H, cf * __restrict__ Y,
	int B, int64_t J, int64_t Jx, int64_t K, int64_t tiles, int bpr, int64_t ir_used )
	{
	const int64_t b = blockIdx.x;
	const int64_t rest = b / bpr;
	const int bin = int( b - rest * bpr ) * CONV_DELAY_THREADS + int( threadIdx.x );
	const int64_t c = rest / tiles, tile = rest - c * tiles;
	if( bin >= B ) return;
	const int64_t j0 = tile * T;
	const cf * Xc = X + c * J * B + bin;
	const cf * Hc = H + ( c % ir_used ) * K * B + bin;
	cf xs[T], acc[T];
	#pragma unroll
	for( int t = 0; t < T; ++t )
		{
		xs[t] = j0 + t < Jx ? Xc[( j0 + t ) * B] : mk( 0.0f, 0.0f );
		acc[t] = mk( 0.0f, 0.0f );
		}
	const int64_t imax = std::min<int64_t>( j0 + T - 1, K - 1 );
	for( int64_t i0 = 0; i0 <= imax; i0 += T )
		{
		#pragma unroll
		for( int u = 0; u < T; ++u )
			{
			const int64_t i = i0 + u;
			if( i > imax ) break;
			const cf h = Hc[i * B];
			const int64_t jn = j0 - i - 1;
			const cf xn = ( jn >= 0 && jn < Jx ) ? Xc[jn * B] : mk( 0.0f, 0.0f );
			#pragma unroll
			for( int t = 0; t < T; ++t )
				{
				const cf x = xs[( t - u + T ) % T];                  // X_{j0+t-i}
				acc[t].x = __builtin_fmaf( x.x, h.x, acc[t].x );
				acc[t].x = __builtin_fmaf( -x.y, h.y, acc[t].x );
				acc[t].y = __builtin_fmaf( x.x, h.y, acc[t].y );
				acc[t].y = __builtin_fmaf( x.y, h.x, acc[t].y );
				}
			xs[T - 1 - u] = xn;                                      // X_{j0-i-1} takes the slot of X_{j0+T-1-i}, needed no more
			}
		}
	#pragma unroll
	for( int t = 0; t < T; ++t )
		if( j0 + t < J ) Y[( c * J + j0 + t ) * B + bin] = acc[t];
	}

// irfft of 2C points per block (block b -> channel b / J, partition j = b % J), keeping the last C samples: y[jC, (j+1)C) cropped to nout.
// The real merge builds Z = A + iB (A = Y[k] + conj Y[C-k], B = ( Y[k] - conj Y[C-k] ) exp(+2 pi i k / 2C)) stored conjugated, so that the
// forward FFT evaluates the inverse ( ifft(Z) = conj( fft( conj Z ) ), as k_synthesize does, pv_kernels.h); 1 / 2C scales it.
// NORM: the block's max |y| over frames below `end` goes into its slot of d_max (an atomic max on the bits of a non-negative float; NaN
// skipped).
template<int LOG2C, bool NORM>
__global__ __launch_bounds__( CONV_TEAM ) void k_conv_inverse( const cf * __restrict__ Y, int64_t J, int64_t nout, int64_t end,
	float * __restrict__ out, unsigned * d_max, const cf * __restrict__ g_tw, const cf * __restrict__ g_tw2 )
	{
	constexpr int C = 1 << LOG2C;
	__shared__ cf s_mem[padded_len( C ) + C];
	__shared__ float s_red[CONV_TEAM / 64];
	cf * buf = s_mem;
	cf * tw = s_mem + padded_len( C );
	const int lane = threadIdx.x;
	const int64_t ch = int64_t( blockIdx.x ) / J, j = int64_t( blockIdx.x ) - ch * J;
	const cf * row = Y + int64_t( blockIdx.x ) * ( C + 1 );
	for( int k = lane; k < C; k += CONV_TEAM )
		{
		tw[k] = g_tw[k];
		cf xk = row[k], xm = row[C - k];
		if( k == 0 ) { xk.y = 0.0f; xm.y = 0.0f; }
		const float ax = xk.x + xm.x, ay = xk.y - xm.y;
		const float dx = xk.x - xm.x, dy = xk.y + xm.y;
		const cf w2q = g_tw2[k];
		const float c = w2q.x, s = -w2q.y;
		const float bx = __builtin_fmaf( c, dx, -( s * dy ) ), by = __builtin_fmaf( c, dy, s * dx );
		buf[PAD( k )] = mk( ax - by, -( ay + bx ) );
		}
	__syncthreads();
	fft_forward<LOG2C, CONV_TEAM>( buf, tw, lane );
	constexpr float scale = 1.0f / float( 2 * C );
	float * o = out + ch * nout;
	float mx = 0.0f;
	for( int q = C / 2 + lane; q < C; q += CONV_TEAM )
		{
		const cf F = buf[PAD( q )];
		const int64_t t = j * C + 2 * ( q - C / 2 );
		const float y0 = F.x * scale, y1 = -F.y * scale;
		if( t < nout ) o[t] = y0;
		if( t + 1 < nout ) o[t + 1] = y1;
		if constexpr( NORM )
			{
			if( t < end ) mx = fmaxf( mx, fabsf( y0 ) );
			if( t + 1 < end ) mx = fmaxf( mx, fabsf( y1 ) );
			}
		}
	if constexpr( NORM )
		{
		#pragma unroll
		for( int off = 32; off > 0; off >>= 1 ) mx = fmaxf( mx, __shfl_xor( mx, off ) );
		if( ( lane & 63 ) == 0 ) s_red[lane >> 6] = mx;
		__syncthreads();
		if( lane == 0 )
			{
			#pragma unroll
			for( int w = 1; w < CONV_TEAM / 64; ++w ) mx = fmaxf( mx, s_red[w] );
			atomicMax( d_max + ( blockIdx.x % CONV_MAX_SLOTS ) * CONV_SLOT_STRIDE, __float_as_uint( mx ) );
			}
		}
	}

// out *= 1.0f / max, the fp32 reciprocal of modify_volume_in_place( 1.0f / max_sample_mag ) (AudioCombination.cpp:346-350); max 0 gives +inf.
// Every wavefront reduces the 64 slots itself (one load per lane).
__global__ __launch_bounds__( 256 ) void k_conv_scale( float * __restrict__ out, int64_t count, const unsigned * d_max )
	{
	static_assert( CONV_MAX_SLOTS == 64, "one slot per lane" );
	float m = __uint_as_float( d_max[( threadIdx.x & 63 ) * CONV_SLOT_STRIDE] );
	#pragma unroll
	for( int off = 32; off > 0; off >>= 1 ) m = fmaxf( m, __shfl_xor( m, off ) );
	const float r = 1.0f / m;
	for( int64_t i = int64_t( blockIdx.x ) * 256 + threadIdx.x; i < count; i += int64_t( gridDim.x ) * 256 ) out[i] = out[i] * r;
	}

template<int LOG2C>
int launch_conv_ffts( bool inverse, const ConvShape & sh, const float * d_x, int64_t ch, int64_t n, const float * d_h, int64_t m,
	void * ws, float * d_out, int normalize, int64_t end, const Plan & plan, hipStream_t s )
	{
	cf * X = ws_at<cf>( ws, sh.x_off ), * H = ws_at<cf>( ws, sh.h_off ), * Y = ws_at<cf>( ws, sh.y_off );
	unsigned * word = ws_at<unsigned>( ws, sh.word_off );
	const int P = sh.P;
	if( !inverse )
		{
		if( int rc = launch_kernel( __func__, k_conv_spectra<LOG2C>, sh.ir_used * sh.K, CONV_TEAM, 0, s,
			d_h, m, sh.K, sh.K, int64_t( 0 ), P, H, plan.d_tw, plan.d_tw2 ) ) return rc;
		return launch_kernel( __func__, k_conv_spectra<LOG2C>, ch * sh.Jx, CONV_TEAM, 0, s,
			d_x, n, sh.Jx, sh.J, int64_t( P ), 2 * P, X, plan.d_tw, plan.d_tw2 );
		}
	const int64_t nout = n + m;
	if( normalize ) return launch_kernel( __func__, k_conv_inverse<LOG2C, true>, ch * sh.J, CONV_TEAM, 0, s, Y, sh.J, nout, end, d_out, word, plan.d_tw, plan.d_tw2 );
	return launch_kernel( __func__, k_conv_inverse<LOG2C, false>, ch * sh.J, CONV_TEAM, 0, s, Y, sh.J, nout, end, d_out, word, plan.d_tw, plan.d_tw2 );
	}

int launch_conv_ffts_any( bool inverse, const ConvShape & sh, const float * d_x, int64_t ch, int64_t n, const float * d_h, int64_t m,
	void * ws, float * d_out, int normalize, int64_t end, const Plan & plan, hipStream_t s )
	{
	switch( sh.log2P )
		{
		case 7: return launch_conv_ffts<7>( inverse, sh, d_x, ch, n, d_h, m, ws, d_out, normalize, end, plan, s );
		case 8: return launch_conv_ffts<8>( inverse, sh, d_x, ch, n, d_h, m, ws, d_out, normalize, end, plan, s );
		case 9: return launch_conv_ffts<9>( inverse, sh, d_x, ch, n, d_h, m, ws, d_out, normalize, end, plan, s );
		case 10: return launch_conv_ffts<10>( inverse, sh, d_x, ch, n, d_h, m, ws, d_out, normalize, end, plan, s );
		case 11: return launch_conv_ffts<11>( inverse, sh, d_x, ch, n, d_h, m, ws, d_out, normalize, end, plan, s );
		case 12: return launch_conv_ffts<12>( inverse, sh, d_x, ch, n, d_h, m, ws, d_out, normalize, end, plan, s );
		default: set_error( "convolve: unsupported partition %d", sh.P ); return FLANHIP_ERR_UNSUPPORTED;
		}
	}

int conv_check( const void * x, int64_t ch, int64_t n, const void * h, int64_t irch, int64_t m, float sr, const void * out, ConvShape * sh )
	{
	FLANHIP_REQUIRE( x && h && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch > 0 && n > 0 && irch > 0 && m > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( conv_shape( ch, n, irch, m, sh ), FLANHIP_ERR_UNSUPPORTED,
		"shape out of range, or a forced partition that is not a power of two from 128 to 4096" );
	return FLANHIP_OK;
	}

int launch_convolve( const float * d_x, int64_t ch, int64_t n, const float * d_h, int64_t irch, int64_t m, float sr, int normalize,
	float * d_out, void * d_ws, hipStream_t s )
	{
	ConvShape sh;
	if( int rc = conv_check( d_x, ch, n, d_h, irch, m, sr, d_out, &sh ) ) return rc;
	FLANHIP_REQUIRE( d_ws, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	if( int rc = require_device() ) return rc;
	std::shared_ptr<const PlanRef> plan;
	if( int rc = get_plan( 2 * sh.P, 2 * sh.P, &plan ) ) return rc;      // tw [P] and tw2 [P+1] of a 2P-point real transform
	const int64_t nout = n + m;
	const int64_t end = max_magnitude_end( nout, sr );
	if( int rc = launch_conv_ffts_any( false, sh, d_x, ch, n, d_h, m, d_ws, d_out, normalize, end, plan->plan, s ) ) return rc;
	if( normalize ) FLANHIP_CHECK( hipMemsetAsync( ws_at<char>( d_ws, sh.word_off ), 0, CONV_MAX_BYTES, s ) );
	const int B = sh.P + 1;
	const int bpr = ( B + CONV_DELAY_THREADS - 1 ) / CONV_DELAY_THREADS;
	const int64_t tiles = ( sh.J + CONV_T - 1 ) / CONV_T;
	if( int rc = launch_kernel( __func__, k_conv_delay<CONV_T>, ch * tiles * bpr, CONV_DELAY_THREADS, 0, s,
		ws_at<const cf>( d_ws, sh.x_off ), ws_at<const cf>( d_ws, sh.h_off ), ws_at<cf>( d_ws, sh.y_off ), B, sh.J, sh.Jx, sh.K, tiles, bpr, sh.ir_used ) ) return rc;
	if( int rc = launch_conv_ffts_any( true, sh, d_x, ch, n, d_h, m, d_ws, d_out, normalize, end, plan->plan, s ) ) return rc;
	if( !normalize ) return FLANHIP_OK;
	const int64_t count = ch * nout;
	return launch_kernel( __func__, k_conv_scale, std::min<int64_t>( ( count + 255 ) / 256, 8192 ), 256, 0, s, d_out, count, ws_at<const unsigned>( d_ws, sh.word_off ) );
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

int64_t flanhip_convolve_out_frames( int64_t num_frames, int64_t ir_frames )
	{
	if( num_frames <= 0 || ir_frames <= 0 ) return 0;
	return num_frames + ir_frames;
	}

size_t flanhip_convolve_workspace_bytes( int64_t num_channels, int64_t num_frames, int64_t ir_channels, int64_t ir_frames )
	{
	ConvShape sh;
	if( !conv_shape( num_channels, num_frames, ir_channels, ir_frames, &sh ) ) return 0;
	return sh.total;
	}

void flanhip_convolve_debug_partition( int samples )
	{
	t_conv_partition = samples > 0 ? samples : 0;
	}

int flanhip_convolve_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, const float * d_ir, int64_t ir_channels, int64_t ir_frames,
	float sample_rate, int normalize, float * d_out, void * d_workspace, void * stream )
	{
	return launch_convolve( d_audio, num_channels, num_frames, d_ir, ir_channels, ir_frames, sample_rate, normalize, d_out, d_workspace,
		(hipStream_t) stream );
	}

int flanhip_convolve( const float * audio, int64_t num_channels, int64_t num_frames, const float * ir, int64_t ir_channels, int64_t ir_frames,
	float sample_rate, int normalize, float * out, volatile int * cancel )
	{
	ConvShape sh;
	if( int rc = conv_check( audio, num_channels, num_frames, ir, ir_channels, ir_frames, sample_rate, out, &sh ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	const float * d_x = nullptr, * d_h = nullptr; float * d_out = nullptr; void * d_ws = nullptr;
	if( int rc = call.in( audio, sizeof( float ) * size_t( num_channels ) * size_t( num_frames ), &d_x ) ) return rc;
	if( int rc = call.in( ir, sizeof( float ) * size_t( ir_channels ) * size_t( ir_frames ), &d_h ) ) return rc;
	if( int rc = call.out( out, sizeof( float ) * size_t( num_channels ) * size_t( num_frames + ir_frames ), &d_out ) ) return rc;
	if( int rc = call.scratch( sh.total, &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_convolve( d_x, num_channels, num_frames, d_h, ir_channels, ir_frames, sample_rate, normalize, d_out, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

} // extern "C"
