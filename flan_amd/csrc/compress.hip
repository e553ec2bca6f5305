// compress.hip -- Audio::compress (Audio/AudioVolume.cpp:190-278), Audio::modify_volume (:5-44) and Audio::set_volume (:46-67).
// DESIGN.md section 4.14.
//
// The reference's compressor is one sequential loop over all frames: a gain computer (per frame, depends on no other frame) followed by a
// two-stage peak detector, each stage a first-order recurrence.  Here:
//   k_comp_level     per frame: the detector input max( 0, max_c s[c][f] ) (signed: :211-215 take no abs), x_L = x_G - y_G, a_R, a_A
//   stage 1          y_1 = max( x_L, a_R y_1 + ( 1 - a_R ) x_L ): the maps y -> max( c, a y + b ) with a >= 0 are closed under
//                    composition, ( a2 a1, a2 b1 + b2, max( c2, a2 c1 + b2 ) ), identity ( 1, 0, -inf ): a scan
//   stage 2          y_L = a_A y_L + ( 1 - a_A ) y_1: affine maps ( a2 a1, a2 b1 + b2 ): a scan
// Each lane owns a run of consecutive frames.  k_comp_sum1 reduces every run to one map (fp64), scans the maps across the wavefront
// (__shfl_up) and the block (LDS) and leaves the block's total; k_scan_carry scans the block totals (one small block) into the state at
// every block's first frame; k_comp_replay1 scans the block again, hands every lane the state at its run's first frame and REPLAYS the
// run with the reference's own fp32 operations in the reference's order, writing y_1 and summarising stage 2 on the way; k_scan_carry
// again; k_comp_replay2 replays stage 2 and writes c = 10^( -y_L / 20 ).  k_gain_apply multiplies every channel by c.
// Only the state a run starts from comes out of the fp64 scan (rounded to fp32 once); everything else is the sequential fp32 loop.
// Every composition runs in a fixed order and there are no atomics: two calls agree bit for bit, and c does not depend on how many
// channels are scaled.  log10, exp and 10^x are evaluated in fp64 and rounded to fp32 once (what glibc's expf / powf do): the fp32
// device functions are 1 ... 2 ulp off, and one ulp of a_R = 0.9998 is 3e-4 of the release time.
// The geometry, block_scan, load4 / store4, lane_run and k_scan_carry are run_scan.h's; the maps and everything per frame are this file's.
#include "run_scan.h"

namespace flanhip {

namespace {

thread_local int t_comp_run = 0;          // flanhip_compress_debug_run: frames per lane forced for the calling thread (0: the library's choice)

constexpr int64_t COMP_MAX_FRAMES = int64_t( 1 ) << 36;
constexpr int64_t COMP_MAX_CHANNELS = 1 << 20;
constexpr int VOL_MAX_PARTIALS = 1024;    // set_volume: the blocks of k_absmax_partial
constexpr size_t VOL_PARTIAL_OFF = 256;   // word 0 of the workspace: the maximum; the partial maxima start here
constexpr size_t VOL_WS_BYTES = 8192;

struct Map1 { double a, b, c; };          // y -> max( c, a y + b ), a >= 0
struct Map2 { double a, b; };             // y -> a y + b

struct CompLayout
	{
	int run = 0;
	int64_t blocks = 0, npad = 0;
	size_t xl = 0, ar = 0, aa = 0, y1 = 0, gain = 0, tot1 = 0, carry1 = 0, tot2 = 0, carry2 = 0, total = 0;
	};

bool comp_layout( int64_t n, CompLayout * l )
	{
	if( n <= 0 || n > COMP_MAX_FRAMES ) return false;
	l->run = scan_run( t_comp_run );
	l->blocks = scan_blocks( n, l->run );
	l->npad = ( n + 3 ) / 4 * 4;
	const size_t row = sizeof( float ) * size_t( l->npad );
	l->xl = 0; l->ar = row; l->aa = 2 * row; l->y1 = 3 * row; l->gain = 4 * row;
	l->tot1 = 5 * row;
	l->carry1 = l->tot1 + sizeof( Map1 ) * size_t( l->blocks );
	l->tot2 = l->carry1 + sizeof( double ) * size_t( l->blocks );
	l->carry2 = l->tot2 + sizeof( Map2 ) * size_t( l->blocks );
	l->total = l->carry2 + sizeof( double ) * size_t( l->blocks );
	return true;
	}

// ---- the maps -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Map1 identity1() { return Map1{ 1.0, 0.0, -INFINITY }; }
__device__ __forceinline__ Map2 identity2() { return Map2{ 1.0, 0.0 }; }
// `l` after `e`.  An empty floor stays empty whatever a is (0 x -inf would be NaN)
__device__ __forceinline__ Map1 then( const Map1 & e, const Map1 & l )
	{
	Map1 r;
	r.a = l.a * e.a;
	r.b = l.a * e.b + l.b;
	r.c = fmax( l.c, e.c == -INFINITY ? -INFINITY : l.a * e.c + l.b );
	return r;
	}
__device__ __forceinline__ Map2 then( const Map2 & e, const Map2 & l ) { return Map2{ l.a * e.a, l.a * e.b + l.b }; }
__device__ __forceinline__ double apply( const Map1 & m, double y ) { return fmax( m.c, m.a * y + m.b ); }
__device__ __forceinline__ double apply( const Map2 & m, double y ) { return m.a * y + m.b; }
__device__ __forceinline__ Map1 shfl_up( const Map1 & m, int off ) { return Map1{ __shfl_up( m.a, off ), __shfl_up( m.b, off ), __shfl_up( m.c, off ) }; }
__device__ __forceinline__ Map2 shfl_up( const Map2 & m, int off ) { return Map2{ __shfl_up( m.a, off ), __shfl_up( m.b, off ) }; }
__device__ __forceinline__ void set_identity( Map1 & m ) { m = identity1(); }
__device__ __forceinline__ void set_identity( Map2 & m ) { m = identity2(); }

// stage 1 of a run as one map: step f is ( a_R, ( 1 - a_R ) x_L, x_L ), the fp32 values the replay uses, composed in fp64
template<bool VEC>
__device__ __forceinline__ Map1 summarise1( const float * xl, const float * ar, int64_t f0, int len )
	{
	Map1 m = identity1();
	for( int i = 0; i < len; i += 4 )
		{
		float x[4], a[4];
		load4<VEC>( xl, f0 + i, len - i, x );
		load4<VEC>( ar, f0 + i, len - i, a );
		#pragma unroll
		for( int k = 0; k < 4; ++k )
			if( i + k < len )
				m = then( m, Map1{ double( a[k] ), double( 1.0f - a[k] ) * double( x[k] ), double( x[k] ) } );
		}
	return m;
	}

// stage 2 of a run as one map: step f is ( a_A, ( 1 - a_A ) y_1 )
template<bool VEC>
__device__ __forceinline__ Map2 summarise2( const float * y1, const float * aa, int64_t f0, int len )
	{
	Map2 m = identity2();
	for( int i = 0; i < len; i += 4 )
		{
		float y[4], a[4];
		load4<VEC>( y1, f0 + i, len - i, y );
		load4<VEC>( aa, f0 + i, len - i, a );
		#pragma unroll
		for( int k = 0; k < 4; ++k )
			if( i + k < len )
				m = then( m, Map2{ double( a[k] ), double( 1.0f - a[k] ) * double( y[k] ) } );
		}
	return m;
	}

// ---- kernels --------------------------------------------------------------------------------------------------------------------
struct CompParams
	{
	const float * threshold, * ratio, * attack, * release, * knee;    // float[n] on the device, or null: the scalar
	float threshold_c, ratio_c, attack_c, release_c, knee_c;
	};

// exp, log10 and 10^x of an fp32 argument, rounded to fp32 once from the fp64 value
__device__ __forceinline__ float exp_rn( float x ) { return float( exp( double( x ) ) ); }
__device__ __forceinline__ float log10_rn( float x ) { return float( log10( double( x ) ) ); }
__device__ __forceinline__ float exp10_rn( float x ) { return float( exp10( double( x ) ) ); }

// AudioVolume.cpp:227-239, as written
__device__ __forceinline__ float gain_computer( float x_G, float threshold, float knee_width, float ratio )
	{
	const float overshoot = x_G - threshold;
	if( overshoot <= -knee_width / 2.0f ) return x_G;
	else if( overshoot >= knee_width / 2.0f ) return x_G + overshoot * ( 1 / ratio - 1 );
	else
		{
		const float z = overshoot + knee_width / 2.0f;
		return x_G + ( 1 / ratio - 1 ) * z * z / ( 2.0f * knee_width );
		}
	}

// one frame per thread: :211-215 (the SIGNED maximum over the sidechain's channels, from 0; a NaN sample is never taken), :264-269, :242
__global__ __launch_bounds__( SCAN_THREADS ) void k_comp_level( const float * __restrict__ side, int64_t side_ch, int64_t side_n, int64_t n, float sr,
	CompParams p, float * __restrict__ xl, float * __restrict__ ar, float * __restrict__ aa )
	{
	const int64_t f = int64_t( blockIdx.x ) * SCAN_THREADS + threadIdx.x;
	if( f >= n ) return;
	float x = 0.0f;
	for( int64_t c = 0; c < side_ch; ++c )
		{
		const float s = side[c * side_n + f];
		if( x < s ) x = s;
		}
	const float x_G = 20.0f * log10_rn( fmaxf( fabsf( x ), 1e-6f ) );
	const float y_G = gain_computer( x_G, p.threshold ? p.threshold[f] : p.threshold_c, p.knee ? p.knee[f] : p.knee_c, p.ratio ? p.ratio[f] : p.ratio_c );
	xl[f] = x_G - y_G;
	ar[f] = exp_rn( -1.0f / ( ( p.release ? p.release[f] : p.release_c ) * sr ) );
	aa[f] = exp_rn( -1.0f / ( ( p.attack ? p.attack[f] : p.attack_c ) * sr ) );
	}

template<bool VEC>
__global__ __launch_bounds__( SCAN_THREADS ) void k_comp_sum1( const float * __restrict__ xl, const float * __restrict__ ar, int64_t n, int run,
	Map1 * __restrict__ tot )
	{
	__shared__ Map1 s_tot[SCAN_WAVES];
	int64_t f0; int len;
	lane_run( n, run, f0, len );
	Map1 excl, total;
	block_scan( summarise1<VEC>( xl, ar, f0, len ), s_tot, excl, total );
	if( threadIdx.x == 0 ) tot[blockIdx.x] = total;
	}

// Stage 1 replayed (:250 in fp32, std::max( a, b ) = a < b ? b : a), y_1 written, stage 2 summarised
template<bool VEC>
__global__ __launch_bounds__( SCAN_THREADS ) void k_comp_replay1( const float * __restrict__ xl, const float * __restrict__ ar,
	const float * __restrict__ aa, int64_t n, int run, const double * __restrict__ carry1, float * __restrict__ y1_out, Map2 * __restrict__ tot2 )
	{
	__shared__ Map1 s_tot1[SCAN_WAVES];
	__shared__ Map2 s_tot2[SCAN_WAVES];
	int64_t f0; int len;
	lane_run( n, run, f0, len );
	Map1 excl, total;
	block_scan( summarise1<VEC>( xl, ar, f0, len ), s_tot1, excl, total );
	float y_1 = float( apply( excl, carry1[blockIdx.x] ) );
	Map2 m2 = identity2();
	for( int i = 0; i < len; i += 4 )
		{
		float x[4], a[4], A[4], y[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
		load4<VEC>( xl, f0 + i, len - i, x );
		load4<VEC>( ar, f0 + i, len - i, a );
		load4<VEC>( aa, f0 + i, len - i, A );
		#pragma unroll
		for( int k = 0; k < 4; ++k )
			if( i + k < len )
				{
				const float v = a[k] * y_1 + ( 1.0f - a[k] ) * x[k];
				y_1 = x[k] < v ? v : x[k];
				y[k] = y_1;
				m2 = then( m2, Map2{ double( A[k] ), double( 1.0f - A[k] ) * double( y_1 ) } );
				}
		store4<VEC>( y1_out, f0 + i, len - i, y );
		}
	Map2 excl2, total2;
	block_scan( m2, s_tot2, excl2, total2 );
	if( threadIdx.x == 0 ) tot2[blockIdx.x] = total2;
	}

// Stage 2 replayed (:251 in fp32) and :272: c = pow( 10.0f, -y_L / 20.0f )
template<bool VEC>
__global__ __launch_bounds__( SCAN_THREADS ) void k_comp_replay2( const float * __restrict__ y1, const float * __restrict__ aa, int64_t n, int run,
	const double * __restrict__ carry2, float * __restrict__ gain )
	{
	__shared__ Map2 s_tot[SCAN_WAVES];
	int64_t f0; int len;
	lane_run( n, run, f0, len );
	Map2 excl, total;
	block_scan( summarise2<VEC>( y1, aa, f0, len ), s_tot, excl, total );
	float y_L = float( apply( excl, carry2[blockIdx.x] ) );
	for( int i = 0; i < len; i += 4 )
		{
		float y[4], A[4], c[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
		load4<VEC>( y1, f0 + i, len - i, y );
		load4<VEC>( aa, f0 + i, len - i, A );
		#pragma unroll
		for( int k = 0; k < 4; ++k )
			if( i + k < len )
				{
				y_L = A[k] * y_L + ( 1.0f - A[k] ) * y[k];
				c[k] = exp10_rn( -y_L / 20.0f );
				}
		store4<VEC>( gain, f0 + i, len - i, c );
		}
	}

// out[ch][f] = in[ch][f] * g[f] for every channel: g = curve[f] (or the scalar), OVER_MAX: divided by *d_max first, one fp32 division
// (:66: level( t ) / max_mag); *d_max == 0 hands the input through (:65).  VEC: four frames per thread, 16 bytes per lane (n a multiple
// of 4 and 16-byte aligned pointers).  out may be in: a thread reads what it writes.
template<bool VEC, bool OVER_MAX>
__global__ __launch_bounds__( 256 ) void k_gain_apply( const float * in, float * out, int64_t ch, int64_t n, const float * curve, float scalar,
	const float * d_max )
	{
	constexpr int W = VEC ? 4 : 1;
	float m = 1.0f;
	if constexpr( OVER_MAX ) m = *d_max;
	const bool through = OVER_MAX && m == 0.0f;
	const int64_t items = n / W;
	for( int64_t q = int64_t( blockIdx.x ) * 256 + threadIdx.x; q < items; q += int64_t( gridDim.x ) * 256 )
		{
		const int64_t f = q * W;
		float g[W];
		if constexpr( VEC )
			{
			if( curve ) { const float4 v = *reinterpret_cast<const float4*>( curve + f ); g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w; }
			else { g[0] = g[1] = g[2] = g[3] = scalar; }
			}
		else g[0] = curve ? curve[f] : scalar;
		if constexpr( OVER_MAX )
			{
			#pragma unroll
			for( int k = 0; k < W; ++k ) g[k] = g[k] / m;
			}
		for( int64_t c = 0; c < ch; ++c )
			{
			if constexpr( VEC )
				{
				float4 v = *reinterpret_cast<const float4*>( in + c * n + f );
				if( !through ) { v.x = v.x * g[0]; v.y = v.y * g[1]; v.z = v.z * g[2]; v.w = v.w * g[3]; }
				*reinterpret_cast<float4*>( out + c * n + f ) = v;
				}
			else
				{
				const float v = in[c * n + f];
				out[c * n + f] = through ? v : v * g[0];
				}
			}
		}
	}

// the block's maximum of one value per thread (256 threads), in thread 0
__device__ __forceinline__ float block_max( float mx, float * s_red )
	{
	#pragma unroll
	for( int off = 32; off > 0; off >>= 1 ) mx = fmaxf( mx, __shfl_xor( mx, off ) );
	if( ( threadIdx.x & 63 ) == 0 ) s_red[threadIdx.x >> 6] = mx;
	__syncthreads();
	return fmaxf( fmaxf( s_red[0], s_red[1] ), fmaxf( s_red[2], s_red[3] ) );
	}

// max |x| over frames [0, end) of every channel: one partial maximum per block (NaN skipped, as std::max( m, |x| ) skips it), no atomics
__global__ __launch_bounds__( 256 ) void k_absmax_partial( const float * __restrict__ in, int64_t ch, int64_t n, int64_t end, float * __restrict__ partial )
	{
	__shared__ float s_red[4];
	float mx = 0.0f;
	for( int64_t f = int64_t( blockIdx.x ) * 256 + threadIdx.x; f < end; f += int64_t( gridDim.x ) * 256 )
		for( int64_t c = 0; c < ch; ++c ) mx = fmaxf( mx, fabsf( in[c * n + f] ) );
	mx = block_max( mx, s_red );
	if( threadIdx.x == 0 ) partial[blockIdx.x] = mx;
	}

__global__ __launch_bounds__( 256 ) void k_absmax_final( const float * __restrict__ partial, int count, float * __restrict__ d_max )
	{
	__shared__ float s_red[4];
	float mx = 0.0f;
	for( int i = threadIdx.x; i < count; i += 256 ) mx = fmaxf( mx, partial[i] );
	mx = block_max( mx, s_red );
	if( threadIdx.x == 0 ) *d_max = mx;
	}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
int launch_gain_apply( const float * d_in, int64_t ch, int64_t n, const float * d_curve, float scalar, const float * d_max, float * d_out, hipStream_t s )
	{
	const bool vec = n % 4 == 0 && aligned16( d_in ) && aligned16( d_out ) && aligned16( d_curve );
	const int64_t items = vec ? n / 4 : n;
	const int64_t blocks = std::min<int64_t>( ( items + 255 ) / 256, int64_t( 1 ) << 20 );
	auto go = [&]( auto kernel ) { return launch_kernel( "launch_gain_apply", kernel, blocks, 256, 0, s, d_in, d_out, ch, n, d_curve, scalar, d_max ); };
	if( vec && d_max ) return go( k_gain_apply<true, true> );
	if( vec ) return go( k_gain_apply<true, false> );
	if( d_max ) return go( k_gain_apply<false, true> );
	return go( k_gain_apply<false, false> );
	}

struct CompArgs
	{
	const float * audio; int64_t ch, n; float sr;
	const float * side; int64_t side_ch, side_n;
	CompParams p;
	float * out, * gain_out;
	};

// what both forms refuse before any device call
int comp_check( const CompArgs & a, CompLayout * l )
	{
	FLANHIP_REQUIRE( a.audio && a.side && a.out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( a.ch > 0 && a.n > 0 && a.side_ch > 0 && a.side_n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( a.sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( a.side_n >= a.n, FLANHIP_ERR_INVALID_ARG, "the sidechain has fewer frames than the audio" );
	FLANHIP_REQUIRE( a.ch <= COMP_MAX_CHANNELS && a.side_ch <= COMP_MAX_CHANNELS && comp_layout( a.n, l ), FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

int launch_compress( const CompArgs & a, void * d_ws, hipStream_t s )
	{
	CompLayout l;
	if( int rc = comp_check( a, &l ) ) return rc;
	FLANHIP_REQUIRE( d_ws, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	if( int rc = require_device() ) return rc;
	float * xl = ws_at<float>( d_ws, l.xl ), * ar = ws_at<float>( d_ws, l.ar ), * aa = ws_at<float>( d_ws, l.aa );
	float * y1 = ws_at<float>( d_ws, l.y1 ), * gain = ws_at<float>( d_ws, l.gain );
	Map1 * tot1 = ws_at<Map1>( d_ws, l.tot1 );
	Map2 * tot2 = ws_at<Map2>( d_ws, l.tot2 );
	double * carry1 = ws_at<double>( d_ws, l.carry1 ), * carry2 = ws_at<double>( d_ws, l.carry2 );
	const int64_t n = a.n;
	// one launch of SCAN_THREADS threads per block; a scan kernel comes as its { 16-byte loads, plain } pair
	auto go = [&]( auto kernel, int64_t blocks, auto... args ) { return launch_kernel( "launch_compress", kernel, blocks, SCAN_THREADS, 0, s, args... ); };
	const bool vec = l.run % 4 == 0 && aligned16( d_ws );        // every run then starts on a 16-byte boundary of the padded rows
	if( int rc = go( k_comp_level, ( n + SCAN_THREADS - 1 ) / SCAN_THREADS, a.side, a.side_ch, a.side_n, n, a.sr, a.p, xl, ar, aa ) ) return rc;
	if( int rc = scan_pair( vec, [&]( auto V ) { return go( k_comp_sum1<V.value>, l.blocks, xl, ar, n, l.run, tot1 ); } ) ) return rc;
	if( int rc = go( k_scan_carry<Map1, double>, 1, tot1, l.blocks, carry1 ) ) return rc;
	if( int rc = scan_pair( vec, [&]( auto V ) { return go( k_comp_replay1<V.value>, l.blocks, xl, ar, aa, n, l.run, carry1, y1, tot2 ); } ) ) return rc;
	if( int rc = go( k_scan_carry<Map2, double>, 1, tot2, l.blocks, carry2 ) ) return rc;
	if( int rc = scan_pair( vec, [&]( auto V ) { return go( k_comp_replay2<V.value>, l.blocks, y1, aa, n, l.run, carry2, gain ); } ) ) return rc;
	if( a.gain_out ) FLANHIP_CHECK( hipMemcpyAsync( a.gain_out, gain, sizeof( float ) * size_t( n ), hipMemcpyDeviceToDevice, s ) );
	return launch_gain_apply( a.audio, a.ch, n, gain, 0.0f, nullptr, a.out, s );
	}

int gain_check( const void * audio, int64_t ch, int64_t n, const void * out )
	{
	FLANHIP_REQUIRE( audio && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch > 0 && n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( ch <= COMP_MAX_CHANNELS && n <= COMP_MAX_FRAMES, FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

size_t flanhip_compress_workspace_bytes( int64_t num_frames )
	{
	CompLayout l;
	if( !comp_layout( num_frames, &l ) ) return 0;
	return l.total;
	}

void flanhip_compress_debug_run( int frames )
	{
	t_comp_run = frames > 0 ? frames : 0;
	}

int flanhip_compress_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * d_sidechain, int64_t side_channels, int64_t side_frames,
	const float * d_threshold, float threshold, const float * d_ratio, float ratio, const float * d_attack, float attack,
	const float * d_release, float release, const float * d_knee_width, float knee_width,
	float * d_out, float * d_gain_out, void * d_workspace, void * stream )
	{
	const CompArgs a{ d_audio, num_channels, num_frames, sample_rate, d_sidechain, side_channels, side_frames,
		CompParams{ d_threshold, d_ratio, d_attack, d_release, d_knee_width, threshold, ratio, attack, release, knee_width }, d_out, d_gain_out };
	return launch_compress( a, d_workspace, (hipStream_t) stream );
	}

int flanhip_compress( const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * sidechain, int64_t side_channels, int64_t side_frames,
	const float * threshold_curve, float threshold, const float * ratio_curve, float ratio, const float * attack_curve, float attack,
	const float * release_curve, float release, const float * knee_width_curve, float knee_width,
	float * out, float * gain_out, volatile int * cancel )
	{
	CompArgs a{ audio, num_channels, num_frames, sample_rate, sidechain, side_channels, side_frames,
		CompParams{ nullptr, nullptr, nullptr, nullptr, nullptr, threshold, ratio, attack, release, knee_width }, out, gain_out };
	CompLayout l;
	if( int rc = comp_check( a, &l ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	const size_t x_bytes = sizeof( float ) * size_t( num_channels ) * size_t( num_frames );
	const size_t row = sizeof( float ) * size_t( num_frames );
	const bool own_side = sidechain == audio && side_channels == num_channels && side_frames == num_frames;
	HostCall call( cancel );
	void * d_ws = nullptr;
	if( int rc = call.in( audio, x_bytes, &a.audio ) ) return rc;
	a.side = a.audio;
	if( !own_side ) if( int rc = call.in( sidechain, sizeof( float ) * size_t( side_channels ) * size_t( side_frames ), &a.side ) ) return rc;
	a.gain_out = nullptr;
	if( gain_out ) if( int rc = call.out( gain_out, row, &a.gain_out ) ) return rc;
	if( int rc = call.out( out, x_bytes, &a.out ) ) return rc;
	if( int rc = call.scratch( l.total, &d_ws ) ) return rc;
	const float * curves[5] = { threshold_curve, ratio_curve, attack_curve, release_curve, knee_width_curve };
	const float ** slots[5] = { &a.p.threshold, &a.p.ratio, &a.p.attack, &a.p.release, &a.p.knee };
	for( int i = 0; i < 5; ++i )
		if( curves[i] ) if( int rc = call.in( curves[i], row, slots[i] ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_compress( a, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

int flanhip_audio_gain_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, const float * d_gain, float gain, float * d_out, void * stream )
	{
	if( int rc = gain_check( d_audio, num_channels, num_frames, d_out ) ) return rc;
	if( int rc = require_device() ) return rc;
	return launch_gain_apply( d_audio, num_channels, num_frames, d_gain, gain, nullptr, d_out, (hipStream_t) stream );
	}

size_t flanhip_audio_set_volume_workspace_bytes( int64_t num_channels, int64_t num_frames )
	{
	if( num_channels <= 0 || num_frames <= 0 || num_channels > COMP_MAX_CHANNELS || num_frames > COMP_MAX_FRAMES ) return 0;
	return VOL_WS_BYTES;
	}

int flanhip_audio_set_volume_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate, const float * d_level, float level,
	float * d_out, void * d_workspace, void * stream )
	{
	if( int rc = gain_check( d_audio, num_channels, num_frames, d_out ) ) return rc;
	FLANHIP_REQUIRE( sample_rate > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	if( int rc = require_device() ) return rc;
	hipStream_t s = (hipStream_t) stream;
	static_assert( VOL_PARTIAL_OFF + sizeof( float ) * VOL_MAX_PARTIALS <= VOL_WS_BYTES, "the partial maxima fit" );
	float * d_max = ws_at<float>( d_workspace, 0 );
	float * partial = ws_at<float>( d_workspace, VOL_PARTIAL_OFF );
	const int64_t end = max_magnitude_end( num_frames, sample_rate );
	const int blocks = int( std::clamp<int64_t>( ( end + 255 ) / 256, 1, VOL_MAX_PARTIALS ) );
	if( int rc = launch_kernel( __func__, k_absmax_partial, blocks, 256, 0, s, d_audio, num_channels, num_frames, end, partial ) ) return rc;
	if( int rc = launch_kernel( __func__, k_absmax_final, 1, 256, 0, s, partial, blocks, d_max ) ) return rc;
	return launch_gain_apply( d_audio, num_channels, num_frames, d_level, level, d_max, d_out, s );
	}

} // extern "C"
