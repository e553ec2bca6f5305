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
//
// Audio::filter_2pole_lowpass / _bandpass / _highpass / _notch (:520-624), filter_2pole_lowshelf / _bandshelf / _highshelf (:631-758) and
// filter_1pole_lowshelf / _highshelf (:431-512) are cascades of the same two sections.  DESIGN.md section 4.16.  What they add: the damping
// R and the cutoff of EVERY section change per frame (k_filt2_coef writes the rows g, R and m of one section, one thread per frame, from
// the cutoff, the damping and the gain by filt2_frame; with three constants the host evaluates filt2_frame itself and no row is
// written), and a section's output is a tap or a fixed mix of its three outputs with a per-frame M or M^2 (FRAME = true below).  The state
// map depends on g and R alone, so the maps, the scan and k_scan_carry are the ones above.
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
	float R;          // the 2-pole section's damping (FRAME: where there is no row R)
	int tap;          // TAP_* or, FRAME only, MIX_*
	float m;          // FRAME: the mix's M or M^2 where there is no row m
	};
// a section's output.  Taps: the low output; the high output (x - lp of a 1-pole section, hp of a 2-pole one); FRAME only: bp * 2 * R with
// the frame's R (:181).  Mixes (FRAME only), f = { lp, bp * 2 * R, hp }, in the reference's order, one rounding per operation:
//   MIX_TILT1      lp * M + ( x - lp ) / M                          (:474, a 1-pole section; m = M)
//   MIX_TILT2      ( f0 / M2 + f1 ) + f2 * M2                       (:482; m = M2 = M * M here and below)
//   MIX_LOWSHELF   ( f0 / ( M2 * M2 ) + f1 / M2 ) + f2              (:721)
//   MIX_HIGHSHELF  ( f0 + f1 * M2 ) + ( f2 * M2 ) * M2              (:755)
//   MIX_BANDSHELF  ( f0 + f1 / M2 ) + f2                            (:738)
enum { TAP_LOW = 0, TAP_HIGH = 1, TAP_BAND = 2, MIX_TILT1 = 3, MIX_TILT2 = 4, MIX_LOWSHELF = 5, MIX_HIGHSHELF = 6, MIX_BANDSHELF = 7 };

struct Map1 { double a, b; };                             // s -> a s + b
struct Map2 { double a11, a12, a21, a22, b1, b2; };       // ( s1, s2 ) -> A ( s1, s2 ) + b
struct State { double s1, s2; };                          // a 1-pole section uses s1
template<int POLES> struct MapOf { using type = Map1; };
template<> struct MapOf<2> { using type = Map2; };

struct FiltLayout
	{
	int run = 0;
	int64_t blocks = 0;                   // per channel
	size_t g = 0, R = 0, m = 0, tot = 0, carry = 0, total = 0;
	};

// the workspace: the row g[n] (n rounded up to 4; rows = 3: the rows R and m after it), then per channel and block a total (sized for
// Map2) and a carried state
bool filt_layout( int64_t ch, int64_t n, FiltLayout * l, int rows = 1 )
	{
	if( ch <= 0 || n <= 0 || ch > FILT_MAX_CHANNELS || n > FILT_MAX_FRAMES ) return false;
	l->run = scan_run( t_filt_run );
	l->blocks = scan_blocks( n, l->run );
	if( l->blocks > FILT_MAX_GRID / ch ) return false;
	const size_t units = size_t( ch ) * size_t( l->blocks );
	const size_t row = sizeof( float ) * size_t( ( n + 3 ) / 4 * 4 );
	l->g = 0; l->R = row; l->m = 2 * row;
	l->tot = size_t( rows ) * row;
	l->carry = l->tot + sizeof( Map2 ) * units;
	l->total = l->carry + sizeof( State ) * units;
	return true;
	}

// ---- the per-frame arithmetic, as the reference writes it -------------------------------------------------------------------------
// :120 std::clamp( c, 1.0f, sr / 2.0f ): two comparisons, a NaN stays; :29 w = tan( T_half c ) / T_half; :67 g = w T_half
__host__ __device__ __forceinline__ float filt_clamp( float cutoff, float nyquist ) { return cutoff < 1.0f ? 1.0f : nyquist < cutoff ? nyquist : cutoff; }
__host__ __device__ __forceinline__ float filt_g_unclamped( float c, float T_half )
	{
	const float w = float( tan( double( T_half * c ) ) ) / T_half;
	return w * T_half;
	}
__host__ __device__ __forceinline__ float filt_g( float cutoff, float T_half, float nyquist ) { return filt_g_unclamped( filt_clamp( cutoff, nyquist ), T_half ); }

// ---- the per-frame values of one section of the filter_2pole_* and shelf cascades -----------------------------------
// Every transcendental is the fp64 function of the fp32 argument rounded to fp32 once; complex products and quotients are the textbook
// forms, one rounding per operation.
enum { ROLE_TILT_1POLE, ROLE_TILT_2POLE, ROLE_REAL_POLE, ROLE_POLE_TIMES, ROLE_POLE_OVER, ROLE_AMP };
struct Filt2Role
	{
	int kind, order;
	int role;         // which section of the cascade: the tilt's 1-pole section (:471-475) or one of its 2-pole sections (:477-483); of the 2-pole
	                  // families the section of the real pole (odd orders, :551-555), p1 = pole w scaler (:568-571) or p2 = pole w / scaler
	                  // (:573-576); ROLE_AMP: no section, the 1-pole shelves' final amp( gain / 2 ) (:498, :510)
	float pre, pim;   // the Butterworth pole above the axis the section belongs to (:32-44)
	float T_half, nyquist;
	};
struct Filt2Frame { float g, R, m; };

// defines.h: pow( 10.0f, d / 20.0f )
__host__ __device__ __forceinline__ float filt_amp( float decibel ) { return float( pow( 10.0, double( decibel / 20.0f ) ) ); }

__host__ __device__ inline Filt2Frame filt2_frame( const Filt2Role & r, float cutoff, float damping, float gain )
	{
	const float two_n = float( 2 * r.order ), order = float( r.order );
	if( r.kind == FLANHIP_FILTER2_1POLE_LOWSHELF || r.kind == FLANHIP_FILTER2_1POLE_HIGHSHELF )
		{
		if( r.role == ROLE_AMP ) return Filt2Frame{ 0.0f, 0.0f, filt_amp( gain / 2.0f ) };
		const float M = filt_amp( ( r.kind == FLANHIP_FILTER2_1POLE_HIGHSHELF ? -gain : gain ) / two_n );     // :466, :509
		const float w = M * filt_clamp( cutoff, r.nyquist );                                                  // :453, :468
		const float g = filt_g_unclamped( w, r.T_half );
		if( r.role == ROLE_TILT_1POLE ) return Filt2Frame{ g, 0.0f, M };
		return Filt2Frame{ g, r.pre / w, M * M };                                                             // :479, :467
		}
	float w, R, M = 1.0f;
	if( r.kind <= FLANHIP_FILTER2_NOTCH ) { w = filt_clamp( cutoff, r.nyquist ); R = damping; }               // :534-535, :545-546
	else
		{
		const bool band = r.kind == FLANHIP_FILTER2_BANDSHELF;
		M = filt_amp( ( band ? -gain : gain / 2.0f ) / two_n );                                               // :647, :720, :737, :754
		w = band ? cutoff : cutoff * M;                                                                       // :718, :735, :752: no clamp
		R = band ? damping * M : damping;
		}
	const float alpha = float( acos( double( R ) ) ) / order;                                                // :547, :669
	float wk, Rk;
	if( r.role == ROLE_REAL_POLE ) { wk = w; Rk = float( cos( double( alpha ) ) ); }                          // :553, :675
	else
		{
		float c, d;                                                                                           // the scaler c + i d (:561-563)
		if( R > 1.0f ) { c = float( pow( double( R + float( sqrt( double( R * R - 1.0f ) ) ) ), double( 1.0f / order ) ) ); d = 0.0f; }
		else { c = float( cos( double( -alpha ) ) ); d = float( sin( double( -alpha ) ) ); }
		const float a = r.pre * w, b = r.pim * w;                                                             // :565
		float re, im;
		if( r.role == ROLE_POLE_TIMES ) { re = a * c - b * d; im = a * d + b * c; }                           // :568
		else { const float den = c * c + d * d; re = ( a * c + b * d ) / den; im = ( b * c - a * d ) / den; } // :573
		wk = float( hypot( double( re ), double( im ) ) );                                                    // :569, :574
		Rk = -re / wk;                                                                                        // :570, :575
		}
	return Filt2Frame{ filt_g_unclamped( wk, r.T_half ), Rk, M * M };
	}

// what a section's step needs of g (and R), in fp32: { G, - } or { g1, d }
template<int POLES>
__device__ __forceinline__ void step_coef( float g, float R, float & p, float & q )
	{
	if constexpr( POLES == 1 ) { p = g / ( 1.0f + g ); q = 0.0f; }                                      // :68
	else { p = 2.0f * R + g; q = 1.0f / ( 1.0f + 2.0f * R * g + g * g ); }                             // :171-172
	}

// one frame of a section in fp32, one rounding per operation: the state moves on, the section's outputs come back (a 1-pole section has lp)
struct Outs { float lp, bp, hp; };
template<int POLES>
__device__ __forceinline__ Outs advance( float x, float g, float R, float & s1, float & s2 )
	{
	float p, q;
	step_coef<POLES>( g, R, p, q );
	if constexpr( POLES == 1 )
		{
		const float v = p * ( x - s1 );                     // :69-71
		const float lp = v + s1;
		s1 = lp + v;
		return Outs{ lp, 0.0f, 0.0f };
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
		return Outs{ lp, bp, hp };
		}
	}

// the frame's output where the tap is TAP_LOW or TAP_HIGH
template<int POLES>
__device__ __forceinline__ float step( float x, float g, float R, int tap, float & s1, float & s2 )
	{
	const Outs o = advance<POLES>( x, g, R, s1, s2 );
	if constexpr( POLES == 1 ) return tap ? x - o.lp : o.lp;          // :73
	else return tap ? o.hp : o.lp;
	}

// the frame's output for any FilterSection::tap, with the frame's own R and m
template<int POLES>
__device__ __forceinline__ float step_frame( float x, float g, float R, float m, int tap, float & s1, float & s2 )
	{
	const Outs o = advance<POLES>( x, g, R, s1, s2 );
	if constexpr( POLES == 1 )
		{
		if( tap == MIX_TILT1 ) return o.lp * m + ( x - o.lp ) / m;
		return tap == TAP_LOW ? o.lp : x - o.lp;
		}
	else
		{
		if( tap == TAP_LOW ) return o.lp;
		if( tap == TAP_HIGH ) return o.hp;
		const float band = o.bp * 2.0f * R;                 // :181
		switch( tap )
			{
			case MIX_TILT2: return o.lp / m + band + o.hp * m;
			case MIX_LOWSHELF: return o.lp / ( m * m ) + band / m + o.hp;
			case MIX_HIGHSHELF: return o.lp + band * m + o.hp * m * m;
			case MIX_BANDSHELF: return o.lp + band / m + o.hp;
			default: return band;
			}
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

// a run of a section as one map: the steps composed in frame order.  g: the row of k_filt_coef, or null for the scalar g_c.  FRAME: R
// per frame as well, from the row R_row or (null) the scalar R
template<int POLES, bool VEC, bool FRAME>
__device__ __forceinline__ typename MapOf<POLES>::type summarise( const float * x_row, const float * g_row, float g_c, const float * R_row, float R, int64_t f0, int len )
	{
	typename MapOf<POLES>::type m;
	set_identity( m );
	for( int i = 0; i < len; i += 4 )
		{
		float x[4], g[4] = { g_c, g_c, g_c, g_c }, Rs[4] = { R, R, R, R };
		load4<VEC>( x_row, f0 + i, len - i, x );
		if( g_row ) load4<VEC>( g_row, f0 + i, len - i, g );
		if constexpr( FRAME && POLES == 2 ) if( R_row ) load4<VEC>( R_row, f0 + i, len - i, Rs );
		#pragma unroll
		for( int k = 0; k < 4; ++k )
			if( i + k < len )
				{
				if constexpr( POLES == 1 ) m = then( m, step_map1( x[k], g[k] ) );
				else m = then( m, step_map2( x[k], g[k], Rs[k] ) );
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

// one frame per thread: the rows g, R and m of the section `role` from the cutoff, the damping and the gain, each a row or (null) a scalar
__global__ __launch_bounds__( SCAN_THREADS ) void k_filt2_coef( Filt2Role role, int64_t n, const float * __restrict__ cutoff, float cutoff_c,
	const float * __restrict__ damping, float damping_c, const float * __restrict__ gain, float gain_c,
	float * __restrict__ g, float * __restrict__ R, float * __restrict__ m )
	{
	const int64_t f = int64_t( blockIdx.x ) * SCAN_THREADS + threadIdx.x;
	if( f >= n ) return;
	const Filt2Frame v = filt2_frame( role, cutoff ? cutoff[f] : cutoff_c, damping ? damping[f] : damping_c, gain ? gain[f] : gain_c );
	g[f] = v.g; R[f] = v.R; m[f] = v.m;
	}

// The rows of a section beside g, each a row or null for the scalar in FilterSection.  FRAME = false (filter_1pole_*): the scalar sec.R
// and the taps TAP_LOW / TAP_HIGH, and these are not read
struct FrameRows { const float * R, * m; };

template<int POLES, bool VEC, bool FRAME>
__global__ __launch_bounds__( SCAN_THREADS ) void k_filt_sum( const float * __restrict__ src, int64_t n, int run, int64_t blocks,
	const float * __restrict__ g_row, float g_c, FrameRows rows, FilterSection sec, typename MapOf<POLES>::type * __restrict__ tot )
	{
	using M = typename MapOf<POLES>::type;
	__shared__ M s_tot[SCAN_WAVES];
	int64_t channel, f0; int len;
	lane_run( n, run, blocks, channel, f0, len );
	M excl, total;
	block_scan( summarise<POLES, VEC, FRAME>( src + channel * n, g_row, g_c, rows.R, sec.R, f0, len ), s_tot, excl, total );
	if( threadIdx.x == 0 ) tot[blockIdx.x] = total;
	}

// The section replayed in fp32 from the carried-in state, its output written.  dst may be src: a lane has read its run when it
// writes it, and reads no other
template<int POLES, bool VEC, bool FRAME>
__global__ __launch_bounds__( SCAN_THREADS ) void k_filt_replay( const float * src, float * dst, int64_t n, int run, int64_t blocks,
	const float * __restrict__ g_row, float g_c, FrameRows rows, FilterSection sec, const State * __restrict__ carry )
	{
	using M = typename MapOf<POLES>::type;
	__shared__ M s_tot[SCAN_WAVES];
	int64_t channel, f0; int len;
	lane_run( n, run, blocks, channel, f0, len );
	const float * x_row = src + channel * n;
	float * y_row = dst + channel * n;
	M excl, total;
	block_scan( summarise<POLES, VEC, FRAME>( x_row, g_row, g_c, rows.R, sec.R, f0, len ), s_tot, excl, total );
	const State start = apply( excl, carry[blockIdx.x] );
	float s1 = float( start.s1 ), s2 = float( start.s2 );
	for( int i = 0; i < len; i += 4 )
		{
		float x[4], g[4] = { g_c, g_c, g_c, g_c }, y[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
		load4<VEC>( x_row, f0 + i, len - i, x );
		if( g_row ) load4<VEC>( g_row, f0 + i, len - i, g );
		if constexpr( FRAME )
			{
			float Rs[4] = { sec.R, sec.R, sec.R, sec.R }, ms[4] = { sec.m, sec.m, sec.m, sec.m };
			if( POLES == 2 && rows.R ) load4<VEC>( rows.R, f0 + i, len - i, Rs );
			if( rows.m ) load4<VEC>( rows.m, f0 + i, len - i, ms );
			#pragma unroll
			for( int k = 0; k < 4; ++k )
				if( i + k < len ) y[k] = step_frame<POLES>( x[k], g[k], Rs[k], ms[k], sec.tap, s1, s2 );
			}
		else
			{
			#pragma unroll
			for( int k = 0; k < 4; ++k )
				if( i + k < len ) y[k] = step<POLES>( x[k], g[k], sec.R, sec.tap, s1, s2 );
			}
		store4<VEC>( y_row, f0 + i, len - i, y );
		}
	}

// What follows the cascade, over the scan's own grid (a block covers SCAN_THREADS * run frames of one channel, frame by frame across the
// block).  POST_SCALE: y = x * m[f], one fp32 product as in Audio::modify_volume (:498, :510); POST_NOTCH: y = ( 0 + ( -bp ) ) + x, what
// modify_volume_in_place( -1 ) and Audio::mix leave of the band-pass bp and the input x (:621-623).  y may be x or bp
enum { POST_SCALE, POST_NOTCH };
template<int POST>
__global__ __launch_bounds__( SCAN_THREADS ) void k_filt2_post( const float * x, const float * bp, float * y, int64_t n, int run, int64_t blocks,
	const float * __restrict__ m_row, float m_c )
	{
	const int64_t channel = int64_t( blockIdx.x ) / blocks;
	const int64_t base = ( int64_t( blockIdx.x ) - channel * blocks ) * SCAN_THREADS * run;
	for( int i = 0; i < run; ++i )
		{
		const int64_t f = base + int64_t( i ) * SCAN_THREADS + threadIdx.x;
		if( f >= n ) break;
		const int64_t at = channel * n + f;
		if constexpr( POST == POST_SCALE ) y[at] = x[at] * ( m_row ? m_row[f] : m_c );
		else y[at] = ( 0.0f + ( -bp[at] ) ) + x[at];
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

// 16-byte loads: every run and every channel's row then start on a 16-byte boundary and end on a whole quad
bool filt_vec( const FiltLayout & l, int64_t n, const void * audio, const void * out, const void * d_ws )
	{
	return l.run % 4 == 0 && n % 4 == 0 && aligned16( audio ) && aligned16( out ) && aligned16( d_ws );
	}

// one section over every channel: k_filt_sum -> k_scan_carry -> k_filt_replay
template<bool FRAME, typename Go>
int run_section( Go go, bool vec, const FiltLayout & l, int64_t ch, int64_t n, const float * src, float * dst,
	const float * g_row, float g_c, FrameRows rows, const FilterSection & sec, void * d_ws )
	{
	State * carry = ws_at<State>( d_ws, l.carry );
	const int64_t grid = l.blocks * ch;
	auto with_poles = [&]( auto P )
		{
		using M = typename MapOf<P.value>::type;
		M * tot = ws_at<M>( d_ws, l.tot );
		if( int rc = scan_pair( vec, [&]( auto V ) { return go( k_filt_sum<P.value, V.value, FRAME>, grid, src, n, l.run, l.blocks, g_row, g_c, rows, sec, tot ); } ) ) return rc;
		if( int rc = go( k_scan_carry<M, State>, ch, (const M*) tot, l.blocks, carry ) ) return rc;
		return scan_pair( vec, [&]( auto V ) { return go( k_filt_replay<P.value, V.value, FRAME>, grid, src, dst, n, l.run, l.blocks, g_row, g_c, rows, sec, (const State*) carry ); } );
		};
	return sec.poles == 1 ? with_poles( std::integral_constant<int, 1>{} ) : with_poles( std::integral_constant<int, 2>{} );
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
	const bool vec = filt_vec( l, n, a.audio, a.out, d_ws );
	const float * src = a.audio;
	for( const FilterSection & sec : filt_sections( a.kind, a.order ) )
		{
		if( int rc = run_section<false>( go, vec, l, a.ch, n, src, a.out, g_row, g_c, FrameRows{}, sec, d_ws ) ) return rc;
		src = a.out;
		}
	return FLANHIP_OK;
	}

// ---- filter_2pole_* and the shelves -------------------------------------------------------------------------------------------------
struct Filt2Args
	{
	const float * audio; int64_t ch, n; float sr;
	const float * cutoff; float cutoff_c;
	const float * damping; float damping_c;
	const float * gain; float gain_c;
	int kind, order;
	float * out;
	};

int filt2_check( const Filt2Args & a, FiltLayout * l )
	{
	FLANHIP_REQUIRE( a.audio && a.out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( a.ch > 0 && a.n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( a.sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( a.kind >= FLANHIP_FILTER2_1POLE_LOWSHELF && a.kind <= FLANHIP_FILTER2_HIGHSHELF, FLANHIP_ERR_INVALID_ARG, "unknown filter kind" );
	FLANHIP_REQUIRE( a.order >= 0 && a.order <= FILT_MAX_ORDER, FLANHIP_ERR_INVALID_ARG, "order outside 0 ... 65535" );
	FLANHIP_REQUIRE( filt_layout( a.ch, a.n, l, 3 ), FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

// The cascade of a kind and order: what the kernels are told of every section (poles and output) and what filt2_frame is.  The tilt
// of the 1-pole shelves (:471-483): for odd N a 1-pole section first, then one 2-pole section per Butterworth pole above the axis.  The
// 2-pole families (:551-577, :673-702): for odd N the section of the real pole first, then per pole TWO sections, pole w scaler and
// pole w / scaler; order N is N state-variable sections, all with the same output.
struct Filt2Section { FilterSection sec; Filt2Role role; };
std::vector<Filt2Section> filt2_sections( int kind, int order, float T_half, float nyquist )
	{
	static const int outputs[] = { MIX_TILT2, MIX_TILT2, TAP_LOW, TAP_BAND, TAP_HIGH, TAP_BAND, MIX_LOWSHELF, MIX_BANDSHELF, MIX_HIGHSHELF };
	const bool tilt = kind == FLANHIP_FILTER2_1POLE_LOWSHELF || kind == FLANHIP_FILTER2_1POLE_HIGHSHELF;
	std::vector<Filt2Section> sections;
	auto add = [&]( int poles, int tap, int role, float pre, float pim )
		{
		sections.push_back( Filt2Section{ FilterSection{ poles, 0.0f, tap, 0.0f }, Filt2Role{ kind, order, role, pre, pim, T_half, nyquist } } );
		};
	if( order % 2 ) { if( tilt ) add( 1, MIX_TILT1, ROLE_TILT_1POLE, 0.0f, 0.0f ); else add( 2, outputs[kind], ROLE_REAL_POLE, 0.0f, 0.0f ); }
	const float pi = acosf( -1.0f ), pi2 = pi * 2.0f;
	for( int i = 0; i < order / 2; ++i )
		{
		const float delta = pi2 / float( order * 2 );                                                        // :39-41
		const float theta = delta * float( i ) + pi / 2.0f + delta / 2.0f;
		const float pre = float( cos( double( theta ) ) ), pim = float( sin( double( theta ) ) );
		if( tilt ) add( 2, outputs[kind], ROLE_TILT_2POLE, pre, pim );
		else { add( 2, outputs[kind], ROLE_POLE_TIMES, pre, pim ); add( 2, outputs[kind], ROLE_POLE_OVER, pre, pim ); }
		}
	return sections;
	}

int launch_filter2( Filt2Args a, void * d_ws, hipStream_t s )
	{
	FiltLayout l;
	if( int rc = filt2_check( a, &l ) ) return rc;
	// what a kind does not look at is no curve: the 1-pole shelves have no damping, the Butterworth kinds and the notch no gain
	if( a.kind <= FLANHIP_FILTER2_1POLE_HIGHSHELF ) a.damping = nullptr;
	else if( a.kind <= FLANHIP_FILTER2_NOTCH ) a.gain = nullptr;
	FLANHIP_REQUIRE( d_ws, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	// :621-623: the notch mixes the band-pass with the input, which a cascade run in place has overwritten by then
	FLANHIP_REQUIRE( a.kind != FLANHIP_FILTER2_NOTCH || a.out != a.audio, FLANHIP_ERR_INVALID_ARG, "the notch's out aliases the input" );
	if( int rc = require_device() ) return rc;
	const int64_t n = a.n;
	const bool tilt = a.kind == FLANHIP_FILTER2_1POLE_LOWSHELF || a.kind == FLANHIP_FILTER2_1POLE_HIGHSHELF;
	auto go = [&]( auto kernel, int64_t blocks, auto... args ) { return launch_kernel( "launch_filter2", kernel, blocks, SCAN_THREADS, 0, s, args... ); };
	const float T_half = acosf( -1.0f ) / a.sr, nyquist = a.sr / 2.0f;        // :57
	const bool curves = a.cutoff || a.damping || a.gain;
	float * g = ws_at<float>( d_ws, l.g ), * R = ws_at<float>( d_ws, l.R ), * m = ws_at<float>( d_ws, l.m );
	// the values of one role: the three rows rewritten (any curve), or three scalars from the same expressions on the host
	auto values = [&]( const Filt2Role & role, Filt2Frame * scalars )
		{
		if( curves ) return go( k_filt2_coef, ( n + SCAN_THREADS - 1 ) / SCAN_THREADS, role, n, a.cutoff, a.cutoff_c, a.damping, a.damping_c, a.gain, a.gain_c, g, R, m );
		*scalars = filt2_frame( role, a.cutoff_c, a.damping_c, a.gain_c );
		return int( FLANHIP_OK );
		};
	const bool vec = filt_vec( l, n, a.audio, a.out, d_ws );
	const int64_t grid = l.blocks * a.ch;
	const float * src = a.audio;
	for( const Filt2Section & sc : filt2_sections( a.kind, a.order, T_half, nyquist ) )
		{
		Filt2Frame v{};
		if( int rc = values( sc.role, &v ) ) return rc;
		FilterSection sec = sc.sec;
		sec.R = v.R; sec.m = v.m;
		const FrameRows rows{ curves ? R : nullptr, curves && sec.tap >= MIX_TILT1 ? m : nullptr };       // a tap reads no m
		if( int rc = run_section<true>( go, vec, l, a.ch, n, src, a.out, curves ? g : nullptr, v.g, rows, sec, d_ws ) ) return rc;
		src = a.out;
		}
	if( a.kind == FLANHIP_FILTER2_NOTCH )                                    // order 0: the band-pass is a copy (:528), so silence
		return go( k_filt2_post<POST_NOTCH>, grid, a.audio, src, a.out, n, l.run, l.blocks, (const float*) nullptr, 0.0f );
	if( tilt )                                                               // order 0: the copy (:447) times amp( gain / 2 )
		{
		Filt2Frame v{};
		if( int rc = values( Filt2Role{ a.kind, a.order, ROLE_AMP, 0.0f, 0.0f, T_half, nyquist }, &v ) ) return rc;
		return go( k_filt2_post<POST_SCALE>, grid, src, src, a.out, n, l.run, l.blocks, (const float*) ( curves ? m : nullptr ), v.m );
		}
	if( a.order == 0 && a.out != a.audio )                                   // :528, :640
		FLANHIP_CHECK( hipMemcpyAsync( a.out, a.audio, sizeof( float ) * size_t( a.ch ) * size_t( n ), hipMemcpyDeviceToDevice, s ) );
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

size_t flanhip_filter2_workspace_bytes( int64_t num_channels, int64_t num_frames )
	{
	FiltLayout l;
	if( !filt_layout( num_channels, num_frames, &l, 3 ) ) return 0;
	return l.total;
	}

int flanhip_filter2_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * d_cutoff, float cutoff, const float * d_damping, float damping, const float * d_gain, float gain,
	int kind, int order, float * d_out, void * d_workspace, void * stream )
	{
	const Filt2Args a{ d_audio, num_channels, num_frames, sample_rate, d_cutoff, cutoff, d_damping, damping, d_gain, gain, kind, order, d_out };
	return launch_filter2( a, d_workspace, (hipStream_t) stream );
	}

int flanhip_filter2( const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * cutoff_curve, float cutoff, const float * damping_curve, float damping, const float * gain_curve, float gain,
	int kind, int order, float * out, volatile int * cancel )
	{
	Filt2Args a{ audio, num_channels, num_frames, sample_rate, nullptr, cutoff, nullptr, damping, nullptr, gain, kind, order, out };
	FiltLayout l;
	if( int rc = filt2_check( a, &l ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	const size_t x_bytes = sizeof( float ) * size_t( num_channels ) * size_t( num_frames ), row_bytes = sizeof( float ) * size_t( num_frames );
	HostCall call( cancel );
	void * d_ws = nullptr;
	if( int rc = call.in( audio, x_bytes, &a.audio ) ) return rc;
	if( int rc = call.out( out, x_bytes, &a.out ) ) return rc;
	if( int rc = call.scratch( l.total, &d_ws ) ) return rc;
	if( cutoff_curve ) if( int rc = call.in( cutoff_curve, row_bytes, &a.cutoff ) ) return rc;
	if( damping_curve ) if( int rc = call.in( damping_curve, row_bytes, &a.damping ) ) return rc;
	if( gain_curve ) if( int rc = call.in( gain_curve, row_bytes, &a.gain ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_filter2( a, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

} // extern "C"
