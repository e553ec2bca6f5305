// filter.hip -- Audio::filter_1pole_lowpass / filter_1pole_highpass (Audio/AudioFilter.cpp:327-387) and filter_1pole_repeat_low /
// filter_1pole_repeat_high (:280-324): cascades of TPT sections with a per-frame cutoff.  DESIGN.md section 4.15.
//
// The reference runs one sequential loop over all frames per channel: every frame goes through the cascade's sections in turn, each a
// 1-pole (:61-74, state s) or a 2-pole state-variable section (:164-182, states s1, s2).  A section is linear in its state:
//   1-pole           s' = ( 1 - 2 G ) s + 2 G x,                       G = g / ( 1 + g )
//   2-pole           ( s1, s2 )' = A ( s1, s2 ) + b x,                 A = [[1 - 2 g d g1, -2 g d], [2 g ( 1 - g d g1 ), 1 - 2 g^2 d]],
//                                                                      b = ( 2 g d, 2 g^2 d ), g1 = 2 R + g, d = 1 / ( 1 + 2 R g + g^2 )
// and affine maps compose, ( A2 A1, A2 b1 + b2 ): a section is a scan over frames, and a cascade is its sections one after the other, each
// over the whole signal (section k reads what section k - 1 wrote).  Here:
//   k_filt_coef      per frame, once for all channels and sections: g = ( tan( T_half c ) / T_half ) T_half, c the clamped cutoff
//                    (:19-30, :119-120); skipped for a scalar cutoff, whose g is computed on the host
//   per section      k_filt_sum reduces every lane's run of consecutive frames to one map (fp64, from the fp32 step values the replay
//                    uses), scans the maps across the wavefront (__shfl_up) and the block (LDS) and leaves the block's total;
//                    k_scan_carry (one block per channel) scans the block totals into the state at every block's first frame, from the
//                    state 0 before frame 0; k_filt_replay scans the block again, hands every lane the state at its run's first frame --
//                    rounded to fp32 once -- and REPLAYS the run with the reference's own fp32 operations in the reference's order.
// Launch boundaries order everything: no block waits for another, no flags, no atomics.  Every composition runs in a fixed order: two
// calls agree bit for bit, and a channel's output does not depend on the channels filtered with it.  A lane reads its run before it writes
// it and reads no other lane's, so a section runs in place: `out` is the working row from the second section on, and may be the input.
// tan is the fp64 function of the fp32 product rounded to fp32 once (compress.hip's rule for exp / log10 / pow).
// The geometry, block_scan, load4 / store4, lane_run and k_scan_carry are run_scan.h's, shared with compress.hip; the maps of two and of
// six numbers and everything per frame are this file's.
#include "run_scan.h"

namespace flanhip {

namespace {

thread_local int t_filt_run = 0;          // flanhip_filter_debug_run: frames per lane forced for the calling thread (0: the library's choice)

constexpr int FILT_MAX_ORDER = 65535;
constexpr int64_t FILT_MAX_FRAMES = int64_t( 1 ) << 36;
constexpr int64_t FILT_MAX_CHANNELS = 1 << 20;
constexpr int64_t FILT_MAX_GRID = ( int64_t( 1 ) << 31 ) - 1;      // blocks x channels of one launch

// What the device code is told about a section.  Butterworth and repeat differ only in the list they make of these.
struct FilterSection
	{
	int poles;        // 1: the 1-pole section (:61-74); 2: the 2-pole state-variable section (:164-182)
	float R;          // the 2-pole section's damping
	int tap;          // 0: the low output; 1: the high output (x - lp of a 1-pole section, hp of a 2-pole one)
	};

struct Map1 { double a, b; };                             // s -> a s + b
struct Map2 { double a11, a12, a21, a22, b1, b2; };       // ( s1, s2 ) -> A ( s1, s2 ) + b
struct State { double s1, s2; };                          // a 1-pole section uses s1
template<int POLES> struct MapOf { using type = Map1; };
template<> struct MapOf<2> { using type = Map2; };

struct FiltLayout
	{
	int run = 0;
	int64_t blocks = 0;                   // per channel
	size_t g = 0, tot = 0, carry = 0, total = 0;
	};

// the workspace: the row g[n] (n rounded up to 4), then per channel and block a total (sized for Map2) and a carried state
bool filt_layout( int64_t ch, int64_t n, FiltLayout * l )
	{
	if( ch <= 0 || n <= 0 || ch > FILT_MAX_CHANNELS || n > FILT_MAX_FRAMES ) return false;
	l->run = scan_run( t_filt_run );
	l->blocks = scan_blocks( n, l->run );
	if( l->blocks > FILT_MAX_GRID / ch ) return false;
	const size_t units = size_t( ch ) * size_t( l->blocks );
	l->g = 0;
	l->tot = sizeof( float ) * size_t( ( n + 3 ) / 4 * 4 );
	l->carry = l->tot + sizeof( Map2 ) * units;
	l->total = l->carry + sizeof( State ) * units;
	return true;
	}

// ---- the per-frame arithmetic, as the reference writes it -------------------------------------------------------------------------
// :120 std::clamp( c, 1.0f, sr / 2.0f ): two comparisons, a NaN stays; :29 w = tan( T_half c ) / T_half; :67 g = w T_half
__host__ __device__ __forceinline__ float filt_g( float cutoff, float T_half, float nyquist )
	{
	const float c = cutoff < 1.0f ? 1.0f : nyquist < cutoff ? nyquist : cutoff;
	const float w = float( tan( double( T_half * c ) ) ) / T_half;
	return w * T_half;
	}

// what a section's step needs of g (and R), in fp32: { G, - } or { g1, d }
template<int POLES>
__device__ __forceinline__ void step_coef( float g, float R, float & p, float & q )
	{
	if constexpr( POLES == 1 ) { p = g / ( 1.0f + g ); q = 0.0f; }                                      // :68
	else { p = 2.0f * R + g; q = 1.0f / ( 1.0f + 2.0f * R * g + g * g ); }                             // :171-172
	}

// one frame of a section in fp32, one rounding per operation: the state moves on, the tapped output comes back
template<int POLES>
__device__ __forceinline__ float step( float x, float g, float R, int tap, float & s1, float & s2 )
	{
	float p, q;
	step_coef<POLES>( g, R, p, q );
	if constexpr( POLES == 1 )
		{
		const float v = p * ( x - s1 );                     // :69-71
		const float lp = v + s1;
		s1 = lp + v;
		return tap ? x - lp : lp;                           // :73
		}
	else
		{
		const float hp = ( x - p * s1 - s2 ) * q;           // :173-179
		const float v1 = g * hp;
		const float bp = v1 + s1;
		s1 = bp + v1;
		const float v2 = g * bp;
		const float lp = v2 + s2;
		s2 = lp + v2;
		return tap ? hp : lp;
		}
	}

// the same frame as a map of the state, in fp64 from the fp32 step values
__device__ __forceinline__ Map1 step_map1( float x, float g )
	{
	float G32, unused;
	step_coef<1>( g, 0.0f, G32, unused );
	const double G2 = 2.0 * double( G32 );
	return Map1{ 1.0 - G2, G2 * double( x ) };
	}
__device__ __forceinline__ Map2 step_map2( float x, float g32, float R )
	{
	float g1_32, d32;
	step_coef<2>( g32, R, g1_32, d32 );
	const double g = double( g32 ), g1 = double( g1_32 ), d = double( d32 );
	const double gd = g * d, ggd = g * gd;
	return Map2{ 1.0 - 2.0 * gd * g1, -2.0 * gd, 2.0 * g * ( 1.0 - gd * g1 ), 1.0 - 2.0 * ggd, 2.0 * gd * double( x ), 2.0 * ggd * double( x ) };
	}

// ---- the maps ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void set_identity( Map1 & m ) { m = Map1{ 1.0, 0.0 }; }
__device__ __forceinline__ void set_identity( Map2 & m ) { m = Map2{ 1.0, 0.0, 0.0, 1.0, 0.0, 0.0 }; }
// `l` after `e`
__device__ __forceinline__ Map1 then( const Map1 & e, const Map1 & l ) { return Map1{ l.a * e.a, l.a * e.b + l.b }; }
__device__ __forceinline__ Map2 then( const Map2 & e, const Map2 & l )
	{
	return Map2{ l.a11 * e.a11 + l.a12 * e.a21, l.a11 * e.a12 + l.a12 * e.a22, l.a21 * e.a11 + l.a22 * e.a21, l.a21 * e.a12 + l.a22 * e.a22,
		l.a11 * e.b1 + l.a12 * e.b2 + l.b1, l.a21 * e.b1 + l.a22 * e.b2 + l.b2 };
	}
__device__ __forceinline__ State apply( const Map1 & m, const State & s ) { return State{ m.a * s.s1 + m.b, 0.0 }; }
__device__ __forceinline__ State apply( const Map2 & m, const State & s ) { return State{ m.a11 * s.s1 + m.a12 * s.s2 + m.b1, m.a21 * s.s1 + m.a22 * s.s2 + m.b2 }; }
__device__ __forceinline__ Map1 shfl_up( const Map1 & m, int off ) { return Map1{ __shfl_up( m.a, off ), __shfl_up( m.b, off ) }; }
__device__ __forceinline__ Map2 shfl_up( const Map2 & m, int off )
	{
	return Map2{ __shfl_up( m.a11, off ), __shfl_up( m.a12, off ), __shfl_up( m.a21, off ), __shfl_up( m.a22, off ), __shfl_up( m.b1, off ), __shfl_up( m.b2, off ) };
	}

// a run of a section as one map: the steps composed in frame order.  g: the row of k_filt_coef, or null for the scalar g_c
template<int POLES, bool VEC>
__device__ __forceinline__ typename MapOf<POLES>::type summarise( const float * x_row, const float * g_row, float g_c, float R, int64_t f0, int len )
	{
	typename MapOf<POLES>::type m;
	set_identity( m );
	for( int i = 0; i < len; i += 4 )
		{
		float x[4], g[4] = { g_c, g_c, g_c, g_c };
		load4<VEC>( x_row, f0 + i, len - i, x );
		if( g_row ) load4<VEC>( g_row, f0 + i, len - i, g );
		#pragma unroll
		for( int k = 0; k < 4; ++k )
			if( i + k < len )
				{
				if constexpr( POLES == 1 ) m = then( m, step_map1( x[k], g[k] ) );
				else m = then( m, step_map2( x[k], g[k], R ) );
				}
		}
	return m;
	}

// ---- kernels ----------------------------------------------------------------------------------------------------------------------
// one frame per thread
__global__ __launch_bounds__( SCAN_THREADS ) void k_filt_coef( const float * __restrict__ cutoff, int64_t n, float T_half, float nyquist, float * __restrict__ g )
	{
	const int64_t f = int64_t( blockIdx.x ) * SCAN_THREADS + threadIdx.x;
	if( f < n ) g[f] = filt_g( cutoff[f], T_half, nyquist );
	}

template<int POLES, bool VEC>
__global__ __launch_bounds__( SCAN_THREADS ) void k_filt_sum( const float * __restrict__ src, int64_t n, int run, int64_t blocks,
	const float * __restrict__ g_row, float g_c, FilterSection sec, typename MapOf<POLES>::type * __restrict__ tot )
	{
	using M = typename MapOf<POLES>::type;
	__shared__ M s_tot[SCAN_WAVES];
	int64_t channel, f0; int len;
	lane_run( n, run, blocks, channel, f0, len );
	M excl, total;
	block_scan( summarise<POLES, VEC>( src + channel * n, g_row, g_c, sec.R, f0, len ), s_tot, excl, total );
	if( threadIdx.x == 0 ) tot[blockIdx.x] = total;
	}

// The section replayed in fp32 from the carried-in state, its tapped output written.  dst may be src: a lane has read its run when it
// writes it, and reads no other
template<int POLES, bool VEC>
__global__ __launch_bounds__( SCAN_THREADS ) void k_filt_replay( const float * src, float * dst, int64_t n, int run, int64_t blocks,
	const float * __restrict__ g_row, float g_c, FilterSection sec, const State * __restrict__ carry )
	{
	using M = typename MapOf<POLES>::type;
	__shared__ M s_tot[SCAN_WAVES];
	int64_t channel, f0; int len;
	lane_run( n, run, blocks, channel, f0, len );
	const float * x_row = src + channel * n;
	float * y_row = dst + channel * n;
	M excl, total;
	block_scan( summarise<POLES, VEC>( x_row, g_row, g_c, sec.R, f0, len ), s_tot, excl, total );
	const State start = apply( excl, carry[blockIdx.x] );
	float s1 = float( start.s1 ), s2 = float( start.s2 );
	for( int i = 0; i < len; i += 4 )
		{
		float x[4], g[4] = { g_c, g_c, g_c, g_c }, y[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
		load4<VEC>( x_row, f0 + i, len - i, x );
		if( g_row ) load4<VEC>( g_row, f0 + i, len - i, g );
		#pragma unroll
		for( int k = 0; k < 4; ++k )
			if( i + k < len ) y[k] = step<POLES>( x[k], g[k], sec.R, sec.tap, s1, s2 );
		store4<VEC>( y_row, f0 + i, len - i, y );
		}
	}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
struct FiltArgs
	{
	const float * audio; int64_t ch, n; float sr;
	const float * cutoff; float cutoff_c;
	int kind, order;
	float * out;
	};

// what both forms refuse before any device call
int filt_check( const FiltArgs & a, FiltLayout * l )
	{
	FLANHIP_REQUIRE( a.audio && a.out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( a.ch > 0 && a.n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( a.sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( a.kind >= FLANHIP_FILTER_BUTTERWORTH_LOW && a.kind <= FLANHIP_FILTER_REPEAT_HIGH, FLANHIP_ERR_INVALID_ARG, "unknown filter kind" );
	FLANHIP_REQUIRE( a.order >= 0 && a.order <= FILT_MAX_ORDER, FLANHIP_ERR_INVALID_ARG, "order outside 0 ... 65535" );
	FLANHIP_REQUIRE( filt_layout( a.ch, a.n, l ), FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

// The cascade of a kind and order.  Butterworth (:32-44, :338-365): for odd N a 1-pole section first, then floor( N / 2 ) 2-pole sections
// with R_i = -Re( exp( i theta_i ) ), theta_i = delta i + pi / 2 + delta / 2, delta = pi2 / ( 2 N ) in fp32 (the cosine is the fp64 one
// rounded once).  Repeat (:296-303): `order` 1-pole sections.  Every section taps low, or every section taps high.
std::vector<FilterSection> filt_sections( int kind, int order )
	{
	std::vector<FilterSection> sections;
	const int tap = kind == FLANHIP_FILTER_BUTTERWORTH_HIGH || kind == FLANHIP_FILTER_REPEAT_HIGH ? 1 : 0;
	if( kind == FLANHIP_FILTER_REPEAT_LOW || kind == FLANHIP_FILTER_REPEAT_HIGH )
		{
		sections.assign( size_t( order ), FilterSection{ 1, 0.0f, tap } );
		return sections;
		}
	const float pi = acosf( -1.0f ), pi2 = pi * 2.0f;
	if( order % 2 ) sections.push_back( FilterSection{ 1, 0.0f, tap } );
	for( int i = 0; i < order / 2; ++i )
		{
		const float delta = pi2 / float( order * 2 );
		const float theta = delta * float( i ) + pi / 2.0f + delta / 2.0f;
		sections.push_back( FilterSection{ 2, -float( cos( double( theta ) ) ), tap } );
		}
	return sections;
	}

int launch_filter( const FiltArgs & a, void * d_ws, hipStream_t s )
	{
	FiltLayout l;
	if( int rc = filt_check( a, &l ) ) return rc;
	FLANHIP_REQUIRE( d_ws, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	if( int rc = require_device() ) return rc;
	const int64_t n = a.n;
	const size_t bytes = sizeof( float ) * size_t( a.ch ) * size_t( n );
	const bool repeat = a.kind == FLANHIP_FILTER_REPEAT_LOW || a.kind == FLANHIP_FILTER_REPEAT_HIGH;
	if( a.order == 0 )
		{
		// :337 order 0 is a copy; :289, :299 no repeats leave the zero-initialised output as it is
		if( repeat ) FLANHIP_CHECK( hipMemsetAsync( a.out, 0, bytes, s ) );
		else if( a.out != a.audio ) FLANHIP_CHECK( hipMemcpyAsync( a.out, a.audio, bytes, hipMemcpyDeviceToDevice, s ) );
		return FLANHIP_OK;
		}
	auto go = [&]( auto kernel, int64_t blocks, auto... args ) { return launch_kernel( "launch_filter", kernel, blocks, SCAN_THREADS, 0, s, args... ); };
	const float T_half = acosf( -1.0f ) / a.sr, nyquist = a.sr / 2.0f;        // :57
	const float * g_row = nullptr;
	float g_c = 0.0f;
	if( a.cutoff )
		{
		float * g = ws_at<float>( d_ws, l.g );
		if( int rc = go( k_filt_coef, ( n + SCAN_THREADS - 1 ) / SCAN_THREADS, a.cutoff, n, T_half, nyquist, g ) ) return rc;
		g_row = g;
		}
	else g_c = filt_g( a.cutoff_c, T_half, nyquist );
	Map1 * tot1 = ws_at<Map1>( d_ws, l.tot );
	Map2 * tot2 = ws_at<Map2>( d_ws, l.tot );
	State * carry = ws_at<State>( d_ws, l.carry );
	const int64_t grid = l.blocks * a.ch;
	// 16-byte loads: every run and every channel's row then start on a 16-byte boundary and end on a whole quad
	const bool vec = l.run % 4 == 0 && n % 4 == 0 && aligned16( a.audio ) && aligned16( a.out ) && aligned16( d_ws );
	const float * src = a.audio;
	for( const FilterSection & sec : filt_sections( a.kind, a.order ) )
		{
		if( sec.poles == 1 )
			{
			if( int rc = scan_pair( vec, [&]( auto V ) { return go( k_filt_sum<1, V.value>, grid, src, n, l.run, l.blocks, g_row, g_c, sec, tot1 ); } ) ) return rc;
			if( int rc = go( k_scan_carry<Map1, State>, a.ch, tot1, l.blocks, carry ) ) return rc;
			if( int rc = scan_pair( vec, [&]( auto V ) { return go( k_filt_replay<1, V.value>, grid, src, a.out, n, l.run, l.blocks, g_row, g_c, sec, carry ); } ) ) return rc;
			}
		else
			{
			if( int rc = scan_pair( vec, [&]( auto V ) { return go( k_filt_sum<2, V.value>, grid, src, n, l.run, l.blocks, g_row, g_c, sec, tot2 ); } ) ) return rc;
			if( int rc = go( k_scan_carry<Map2, State>, a.ch, tot2, l.blocks, carry ) ) return rc;
			if( int rc = scan_pair( vec, [&]( auto V ) { return go( k_filt_replay<2, V.value>, grid, src, a.out, n, l.run, l.blocks, g_row, g_c, sec, carry ); } ) ) return rc;
			}
		src = a.out;
		}
	return FLANHIP_OK;
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

size_t flanhip_filter_1pole_workspace_bytes( int64_t num_channels, int64_t num_frames )
	{
	FiltLayout l;
	if( !filt_layout( num_channels, num_frames, &l ) ) return 0;
	return l.total;
	}

void flanhip_filter_debug_run( int frames )
	{
	t_filt_run = frames > 0 ? frames : 0;
	}

int flanhip_filter_1pole_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * d_cutoff, float cutoff, int kind, int order, float * d_out, void * d_workspace, void * stream )
	{
	const FiltArgs a{ d_audio, num_channels, num_frames, sample_rate, d_cutoff, cutoff, kind, order, d_out };
	return launch_filter( a, d_workspace, (hipStream_t) stream );
	}

int flanhip_filter_1pole( const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * cutoff_curve, float cutoff, int kind, int order, float * out, volatile int * cancel )
	{
	FiltArgs a{ audio, num_channels, num_frames, sample_rate, nullptr, cutoff, kind, order, out };
	FiltLayout l;
	if( int rc = filt_check( a, &l ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	const size_t x_bytes = sizeof( float ) * size_t( num_channels ) * size_t( num_frames );
	HostCall call( cancel );
	void * d_ws = nullptr;
	if( int rc = call.in( audio, x_bytes, &a.audio ) ) return rc;
	if( int rc = call.out( out, x_bytes, &a.out ) ) return rc;
	if( int rc = call.scratch( l.total, &d_ws ) ) return rc;
	if( cutoff_curve ) if( int rc = call.in( cutoff_curve, sizeof( float ) * size_t( num_frames ), &a.cutoff ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_filter( a, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

} // extern "C"
