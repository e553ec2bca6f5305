// multinotch.hip -- Audio::filter_1pole_multinotch (Audio/AudioFilter.cpp:802-885) and filter_2pole_multinotch (:887-986) with
// use_saturator == false: an all-pass cascade whose sections are coupled through an instantaneous feedback path.  DESIGN.md section 4.19.
//
// The reference runs one sequential loop per channel.  At every frame, with g = w T_half from the clamped, prewarped cutoff (:814, :829,
// :833), k the feedback, inv = +-1, a = wet_dry, and `order` sections (1-pole :52-84, state s; 2-pole :154-192, states s1, s2):
//   1-pole   G = ( g - 1 ) / ( g + 1 );   M = ( sum_i G^i s[order-1-i] ) 2 / ( 1 + g );               x_bar = ( x + inv k M ) / ( 1 - inv k G^order )
//   2-pole   d = 1 / ( 1 + 2 R g + g g ), G = d ( 1 - 2 R g + g g );   M = sum_i G^i ( g s2 - s1 )[order-1-i];   x_bar = ( x + inv k 4 R d M ) / ( 1 - inv k G^order )
//   then     x_bar runs through the sections in turn, each putting out lp - hp (1-pole) or lp - 2 R bp + hp (2-pole) and moving its state;
//            y_bar = inv * that;   y = a x_bar + ( 1 - a ) y_bar
// Every line is linear in the states and x: with s in R^D (D = order, or 2 order: s1, s2 of section 0, then of section 1 ...) a frame is
// s' = A_t s + b_t x_t.  A_t is a lower-triangular cascade plus a rank-one feedback term and changes every frame; products of such
// matrices have no structure, so the scan element is the dense pair ( A, r ), D x D + D doubles, and
// then( earlier, later ) = ( A_l A_e, A_l r_e + r_l ).  At D = 16 that is 272 doubles: no lane holds it.  Here a TEAM of lanes holds an
// element: D is padded to DP = 4, 8 or 16, a team is 2 DP lanes, lane c < DP holds column c of A, lane DP holds r, the others idle (a
// power of two wide and one column too many for DP lanes).  A team owns a run of consecutive frames; a block of 256 threads has 128 / DP teams.
//   k_mn_coef     one thread per frame, once for all channels: the rows g, R, inv k, a (fp32) and the denominator 1 - inv k G^order (the
//                 reference's double, below); no transcendental is evaluated anywhere else
//   k_mn_sum      every lane of a team runs the frame loop over the team's run in fp64, from the fp32 rows: lane c < D from the unit state
//                 e_c with silence in (column c of A), lane DP from the zero state with the run's input (r).  The block's elements are
//                 then composed in team order by doubling: a team publishes its element in LDS, reads the column it owns of the element
//                 `off` teams before it, and multiplies it by its own matrix, read from LDS as a broadcast.  The last team's is the block's total.
//   k_mn_carry    one block per channel: the totals, 128 / DP at a time, scanned by the same doubling, and the state entering every block from
//                 the state before the pass; the passes follow one another
//   k_mn_replay   the block scanned again, the state at a run's first frame from the element before it and the block's carried state,
//                 rounded to fp32 ONCE; one lane then REPLAYS the run with the reference's own operations in the reference's order (eight
//                 replays share a wavefront; a wavefront left without one retires).
// Launch boundaries order everything: no block waits for another, no flags, no atomics.  Every composition runs in a fixed order: two
// calls agree bit for bit, and a channel's output does not depend on the channels filtered with it.  A team reads its run before the
// block's first barrier and writes it after the last: out may be the audio.  An element is composed from the elements of earlier
// frames alone, so a sample that is not finite reaches no earlier frame and no other channel.
//
// The reference's arithmetic, kept (tan: the fp64 function of the fp32 product rounded once, filter.hip's rule):
//   std::pow( G, i ) with an integer exponent is the DOUBLE function: M += pow * s is a double product and a double sum rounded to float
//   at every term; the denominator 1.0f - inv * k * pow( G, order ) is a double and the quotient is rounded to float once.  Everything
//   else is fp32, one rounding per operation, left to right: inv * k first, the 2-pole numerator ((((inv k) 4) R) d) M.  The powers G^i
//   of the sum are formed here by i fp64 products in the replay (i ulps of fp64 from pow, 2^-25 of an fp32 ulp); G^order of the
//   denominator is pow itself, in k_mn_coef.  Damping and feedback are not clamped.  feedback_sampled of the 1-pole form is dead: it
//   calls its Functions per frame, one value per frame either way.  order == 0 reads an uninitialised y_bar there and is refused
//   here; the saturated form (a Newton iteration on tanh per frame, not linear in the state: no scan) is not offered.
#include "run_scan.h"

namespace flanhip {

namespace {

thread_local int t_mn_run = 0;            // flanhip_multinotch_debug_run: frames per team forced for the calling thread (0: the library's choice)

constexpr int MN_THREADS = 256;
constexpr int MN_RUN_PER_STATE = 16;      // frames per team: 16 DP, so that a block of 128 / DP teams is 2048 frames whatever DP is (1407 blocks per row for a
                                          // minute at 48 kHz): the wider the element, the fewer totals k_mn_carry has to take one pass after the other
constexpr int MN_REPLAYS = 8;             // replays a wavefront of k_mn_replay carries: measured on 8 ch x 60 s, 2 of them in each of four wavefronts (D = 16)
                                          // cost 3.3 ms of 12 more than 8 in one, and 32 in one (D = 4) 0.65 ms of 1.1 more than 8 in each of four
constexpr int MN_MAX_D = 16;
constexpr int64_t MN_MAX_FRAMES = int64_t( 1 ) << 36;
constexpr int64_t MN_MAX_CHANNELS = 1 << 20;
constexpr int64_t MN_MAX_GRID = ( int64_t( 1 ) << 31 ) - 1;

template<int DP> struct Geo
	{
	static constexpr int TW = 2 * DP;                 // lanes of a team
	static constexpr int TEAMS = MN_THREADS / TW;     // of a block, and the elements k_mn_carry scans in one pass
	static constexpr int EL = ( DP + 1 ) * DP;        // doubles of an element: the columns of A, then r
	};

struct MnLayout
	{
	int run = 0, D = 0, DP = 0, teams = 0;
	int64_t blocks = 0;                   // per channel
	size_t den = 0, g = 0, R = 0, ik = 0, mix = 0, tot = 0, carry = 0, total = 0;
	};

// the state dimension of a kind and order: 0 for an order that is not positive, MN_MAX_D + 1 for any order above MN_MAX_D (no overflow)
int mn_dim( int kind, int order )
	{
	if( order <= 0 || order > MN_MAX_D ) return order <= 0 ? 0 : MN_MAX_D + 1;
	return kind == FLANHIP_MULTINOTCH_1POLE ? order : 2 * order;
	}

// the workspace: the row den[n] of doubles and the rows g, R, ik, mix of floats (n rounded up to 4), then per channel and block a total
// of ( DP + 1 ) DP doubles and a carried state of DP doubles
bool mn_layout( int64_t ch, int64_t n, int kind, int order, MnLayout * l )
	{
	if( ch <= 0 || n <= 0 || ch > MN_MAX_CHANNELS || n > MN_MAX_FRAMES ) return false;
	if( kind != FLANHIP_MULTINOTCH_1POLE && kind != FLANHIP_MULTINOTCH_2POLE ) return false;
	l->D = mn_dim( kind, order );
	if( l->D <= 0 || l->D > MN_MAX_D ) return false;
	l->DP = l->D <= 4 ? 4 : l->D <= 8 ? 8 : 16;
	l->teams = MN_THREADS / ( 2 * l->DP );
	l->run = t_mn_run > 0 ? std::min( t_mn_run, SCAN_MAX_RUN ) : MN_RUN_PER_STATE * l->DP;
	const int64_t per_block = int64_t( l->teams ) * l->run;
	l->blocks = ( n + per_block - 1 ) / per_block;
	if( l->blocks > MN_MAX_GRID / ch ) return false;
	const size_t units = size_t( ch ) * size_t( l->blocks ), n4 = size_t( ( n + 3 ) / 4 * 4 );
	l->den = 0;
	l->g = sizeof( double ) * n4;
	l->R = l->g + sizeof( float ) * n4;
	l->ik = l->R + sizeof( float ) * n4;
	l->mix = l->ik + sizeof( float ) * n4;
	l->tot = l->mix + sizeof( float ) * n4;
	l->carry = l->tot + sizeof( double ) * units * size_t( ( l->DP + 1 ) * l->DP );
	l->total = l->carry + sizeof( double ) * units * size_t( l->DP );
	return true;
	}

// ---- the per-frame arithmetic -------------------------------------------------------------------------------------------------------
// :814 std::clamp( c, 1.0f, sr / 2.0f ): two comparisons, a NaN stays; :19-30 w = tan( T_half c ) / T_half; :833 g = w T_half
__device__ __forceinline__ float mn_g( float cutoff, float T_half, float nyquist )
	{
	const float c = cutoff < 1.0f ? 1.0f : nyquist < cutoff ? nyquist : cutoff;
	const float w = float( tan( double( T_half * c ) ) ) / T_half;
	return w * T_half;
	}
// the G of the feedback path in fp32: :834, :934-935
template<int KIND>
__device__ __forceinline__ float mn_G( float g, float R )
	{
	if constexpr( KIND == FLANHIP_MULTINOTCH_1POLE ) return ( g - 1.0f ) / ( g + 1.0f );
	else
		{
		const float d = 1.0f / ( 1.0f + 2.0f * R * g + g * g );
		return d * ( 1.0f - 2.0f * R * g + g * g );
		}
	}

// One frame as the reference runs it (:828-879, :928-981): the states move on, y comes back.  s: s[j] of section j, or s1, s2 of section
// j at [2 j], [2 j + 1]; sections >= order are padding and are not touched.  den: the double 1.0f - inv * k * pow( G, order )
template<int KIND, int DP>
__device__ __forceinline__ float mn_step32( float x, float g, float R, float ik, double den, float mix, float inv, int order, float ( &s )[DP] )
	{
	constexpr int NS = KIND == FLANHIP_MULTINOTCH_1POLE ? DP : DP / 2;
	const double Gd = double( mn_G<KIND>( g, R ) );
	float ms = 0.0f;
	double pw = 1.0;
	float xb;
	if constexpr( KIND == FLANHIP_MULTINOTCH_1POLE )
		{
		#pragma unroll
		for( int j = NS - 1; j >= 0; --j )
			if( j < order ) { ms = float( double( ms ) + pw * double( s[j] ) ); pw = pw * Gd; }          // :837-838
		ms = ms * ( 2.0f / ( 1.0f + g ) );                                                                 // :839
		xb = float( double( x + ik * ms ) / den );                                                         // :867
		const float G = g / ( 1.0f + g );                                                                  // :68
		float y = xb;
		#pragma unroll
		for( int j = 0; j < NS; ++j )
			if( j < order )
				{
				const float v = G * ( y - s[j] );                                                          // :69-73
				const float lp = v + s[j];
				s[j] = lp + v;
				y = lp - ( y - lp );                                                                       // :79 lp * 1 + hp * -1
				}
		return mix * xb + ( 1.0f - mix ) * ( y * inv );                                                    // :876-878
		}
	else
		{
		const float g1 = 2.0f * R + g;                                                                     // :171-172
		const float d = 1.0f / ( 1.0f + 2.0f * R * g + g * g );
		#pragma unroll
		for( int j = NS - 1; j >= 0; --j )
			if( j < order ) { const float t = g * s[2 * j + 1] - s[2 * j]; ms = float( double( ms ) + pw * double( t ) ); pw = pw * Gd; }      // :938-939
		xb = float( double( x + ik * 4.0f * R * d * ms ) / den );                                         // :967
		float y = xb;
		#pragma unroll
		for( int j = 0; j < NS; ++j )
			if( j < order )
				{
				const float hp = ( y - g1 * s[2 * j] - s[2 * j + 1] ) * d;                                 // :173-179
				const float v1 = g * hp;
				const float bp = v1 + s[2 * j];
				s[2 * j] = bp + v1;
				const float v2 = g * bp;
				const float lp = v2 + s[2 * j + 1];
				s[2 * j + 1] = lp + v2;
				y = ( lp - bp * 2.0f * R ) + hp;                                                           // :181, :187 mix { 1, -1, 1 }
				}
		return mix * xb + ( 1.0f - mix ) * ( y * inv );                                                    // :976-979
		}
	}

// The same frame as a map of the state, in fp64 from the fp32 rows g, R and inv k: only the states move
template<int KIND, int DP>
__device__ __forceinline__ void mn_step64( double x, double g, double R, double ik, int order, double ( &s )[DP] )
	{
	constexpr int NS = KIND == FLANHIP_MULTINOTCH_1POLE ? DP : DP / 2;
	double ms = 0.0, pw = 1.0;
	if constexpr( KIND == FLANHIP_MULTINOTCH_1POLE )
		{
		const double q = 1.0 / ( 1.0 + g ), G = g * q, Ga = ( g - 1.0 ) * q;
		#pragma unroll
		for( int j = NS - 1; j >= 0; --j )
			if( j < order ) { ms += pw * s[j]; pw *= Ga; }
		double y = ( x + ik * ( ms * 2.0 * q ) ) / ( 1.0 - ik * pw );
		#pragma unroll
		for( int j = 0; j < NS; ++j )
			if( j < order )
				{
				const double v = G * ( y - s[j] );
				const double lp = v + s[j];
				s[j] = lp + v;
				y = lp - ( y - lp );
				}
		}
	else
		{
		const double g1 = 2.0 * R + g, num = 1.0 + g * g, rg = 2.0 * R * g;
		const double d = 1.0 / ( num + rg ), Ga = d * ( num - rg );
		#pragma unroll
		for( int j = NS - 1; j >= 0; --j )
			if( j < order ) { ms += pw * ( g * s[2 * j + 1] - s[2 * j] ); pw *= Ga; }
		double y = ( x + ik * 4.0 * R * d * ms ) / ( 1.0 - ik * pw );
		#pragma unroll
		for( int j = 0; j < NS; ++j )
			if( j < order )
				{
				const double hp = ( y - g1 * s[2 * j] - s[2 * j + 1] ) * d;
				const double v1 = g * hp;
				const double bp = v1 + s[2 * j];
				s[2 * j] = bp + v1;
				const double v2 = g * bp;
				const double lp = v2 + s[2 * j + 1];
				s[2 * j + 1] = lp + v2;
				y = ( lp - 2.0 * R * bp ) + hp;
				}
		}
	}

struct MnRows { const double * den; const float * g, * R, * ik, * mix; };

// the column of the run's element that lane c of a team holds: c < D column c of A, c == DP r, nothing (zeros) otherwise.  A run with
// no frames (past the row's end) is the identity
template<int KIND, int DP>
__device__ __forceinline__ void mn_summarise( const float * x_row, const MnRows & rows, int64_t f0, int len, int order, int D, int c, double ( &col )[DP] )
	{
	#pragma unroll
	for( int i = 0; i < DP; ++i ) col[i] = i == c ? 1.0 : 0.0;
	if( !( c < D || c == DP ) ) return;
	for( int i = 0; i < len; ++i )
		{
		const int64_t f = f0 + i;
		const double x = c == DP ? double( x_row[f] ) : 0.0;
		mn_step64<KIND, DP>( x, double( rows.g[f] ), double( rows.R[f] ), double( rows.ik[f] ), order, col );
		}
	}

// The elements of the block's teams composed in team order, by doubling.  Every thread of the block calls it with the column it holds;
// it comes back holding the same column of the composition of its team's element with all earlier teams', and the buffer of s_el that
// is returned holds every team's.  Whoever calls it twice puts a barrier between its last read of s_el and the second call
template<int DP>
__device__ __forceinline__ int mn_block_scan( double ( &col )[DP], double ( *s_el )[Geo<DP>::TEAMS][Geo<DP>::EL], int D )
	{
	constexpr int TW = Geo<DP>::TW, TEAMS = Geo<DP>::TEAMS;
	const int t = threadIdx.x / TW, c = threadIdx.x % TW;
	int buf = 0;
	if( c <= DP )
		{
		#pragma unroll
		for( int i = 0; i < DP; ++i ) s_el[0][t][c * DP + i] = col[i];
		}
	__syncthreads();
	for( int off = 1; off < TEAMS; off <<= 1 )
		{
		if( t >= off && c <= DP )
			{
			// mine after the element `off` teams earlier: A_mine applied to the earlier column this lane owns (+ r_mine on the lane of r)
			const double * e = s_el[buf][t - off] + c * DP, * A = s_el[buf][t];
			double acc[DP];
			#pragma unroll
			for( int i = 0; i < DP; ++i ) acc[i] = c == DP ? col[i] : 0.0;
			#pragma unroll
			for( int j = 0; j < DP; ++j )
				if( j < D )
					{
					const double ej = e[j];
					#pragma unroll
					for( int i = 0; i < DP; ++i ) acc[i] += A[j * DP + i] * ej;
					}
			#pragma unroll
			for( int i = 0; i < DP; ++i ) col[i] = acc[i];
			}
		buf ^= 1;
		if( c <= DP )
			{
			#pragma unroll
			for( int i = 0; i < DP; ++i ) s_el[buf][t][c * DP + i] = col[i];
			}
		__syncthreads();
		}
	return buf;
	}

// component i of an element applied to a state: ( A s + r )[i], the terms in column order
template<int DP>
__device__ __forceinline__ double mn_apply( const double * el, const double * state, int D, int i )
	{
	double v = el[DP * DP + i];
	#pragma unroll
	for( int j = 0; j < DP; ++j )
		if( j < D ) v += el[j * DP + i] * state[j];
	return v;
	}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
// one frame per thread, once for all channels; each parameter a row or (null) the scalar
template<int KIND>
__global__ __launch_bounds__( MN_THREADS ) void k_mn_coef( int64_t n, float T_half, float nyquist, const float * __restrict__ cutoff, float cutoff_c,
	const float * __restrict__ damping, float damping_c, const float * __restrict__ feedback, float feedback_c, const float * __restrict__ wet_dry, float wet_dry_c,
	float inv, int order, double * __restrict__ den, float * __restrict__ g_row, float * __restrict__ R_row, float * __restrict__ ik_row, float * __restrict__ mix_row )
	{
	const int64_t f = int64_t( blockIdx.x ) * MN_THREADS + threadIdx.x;
	if( f >= n ) return;
	const float g = mn_g( cutoff ? cutoff[f] : cutoff_c, T_half, nyquist );
	const float R = KIND == FLANHIP_MULTINOTCH_2POLE ? ( damping ? damping[f] : damping_c ) : 0.0f;
	const float ik = inv * ( feedback ? feedback[f] : feedback_c );
	g_row[f] = g; R_row[f] = R; ik_row[f] = ik;
	mix_row[f] = wet_dry ? wet_dry[f] : wet_dry_c;
	den[f] = 1.0 - double( ik ) * pow( double( mn_G<KIND>( g, R ) ), double( order ) );          // :867, :967
	}

template<int KIND, int DP>
__global__ __launch_bounds__( MN_THREADS ) void k_mn_sum( const float * __restrict__ audio, int64_t n, int run, int64_t blocks, int order, int D, MnRows rows,
	double * __restrict__ tot )
	{
	constexpr int TW = Geo<DP>::TW, TEAMS = Geo<DP>::TEAMS, EL = Geo<DP>::EL;
	__shared__ double s_el[2][TEAMS][EL];
	const int t = threadIdx.x / TW, c = threadIdx.x % TW;
	const int64_t channel = int64_t( blockIdx.x ) / blocks, block = int64_t( blockIdx.x ) - channel * blocks;
	const int64_t f0 = ( block * TEAMS + t ) * run;
	const int len = int( std::min<int64_t>( std::max<int64_t>( n - f0, 0 ), run ) );
	double col[DP];
	mn_summarise<KIND, DP>( audio + channel * n, rows, f0, len, order, D, c, col );
	mn_block_scan<DP>( col, s_el, D );
	if( t == TEAMS - 1 && c <= DP )
		{
		double * out = tot + int64_t( blockIdx.x ) * EL + c * DP;
		#pragma unroll
		for( int i = 0; i < DP; ++i ) out[i] = col[i];
		}
	}

// One block per channel: the state at the first frame of every block of the channel's scan, from the block totals and the zero state
// before frame 0.  A pass scans TEAMS totals by doubling; the state after a pass is the state before the next.  tot: [ch][blocks][EL], carry: [ch][blocks][DP]
template<int DP>
__global__ __launch_bounds__( MN_THREADS ) void k_mn_carry( const double * __restrict__ tot, int64_t blocks, int D, double * __restrict__ carry )
	{
	constexpr int TW = Geo<DP>::TW, TEAMS = Geo<DP>::TEAMS, EL = Geo<DP>::EL;
	__shared__ double s_el[2][TEAMS][EL];
	__shared__ double s_state[DP];
	const int t = threadIdx.x / TW, c = threadIdx.x % TW;
	tot += int64_t( blockIdx.x ) * blocks * EL;
	carry += int64_t( blockIdx.x ) * blocks * DP;
	if( threadIdx.x < DP ) s_state[threadIdx.x] = 0.0;
	__syncthreads();
	for( int64_t base = 0; base < blocks; base += TEAMS )
		{
		const int64_t b = base + t;
		double col[DP];
		#pragma unroll
		for( int i = 0; i < DP; ++i ) col[i] = i == c ? 1.0 : 0.0;
		if( b < blocks && c <= DP )
			{
			const double * in = tot + b * EL + c * DP;
			#pragma unroll
			for( int i = 0; i < DP; ++i ) col[i] = in[i];
			}
		const int buf = mn_block_scan<DP>( col, s_el, D );
		if( b < blocks && c < DP ) carry[b * DP + c] = t == 0 ? s_state[c] : mn_apply<DP>( s_el[buf][t - 1], s_state, D, c );
		double next = 0.0;
		if( t == 0 && c < DP ) next = mn_apply<DP>( s_el[buf][TEAMS - 1], s_state, D, c );
		__syncthreads();
		if( t == 0 && c < DP ) s_state[c] = next;
		__syncthreads();
		}
	}

// dst may be src: every lane has read its team's run when the block passes the scan's barriers, and a team writes no other's
template<int KIND, int DP>
__global__ __launch_bounds__( MN_THREADS ) void k_mn_replay( const float * src, float * dst, int64_t n, int run, int64_t blocks, int order, int D, float inv, MnRows rows,
	const double * __restrict__ carry )
	{
	constexpr int TW = Geo<DP>::TW, TEAMS = Geo<DP>::TEAMS, EL = Geo<DP>::EL;
	__shared__ double s_el[2][TEAMS][EL];
	const int t = threadIdx.x / TW, c = threadIdx.x % TW;
	const int64_t channel = int64_t( blockIdx.x ) / blocks, block = int64_t( blockIdx.x ) - channel * blocks;
	const int64_t f0 = ( block * TEAMS + t ) * run;
	const int len = int( std::min<int64_t>( std::max<int64_t>( n - f0, 0 ), run ) );
	const float * x_row = src + channel * n;
	float * y_row = dst + channel * n;
	double col[DP];
	mn_summarise<KIND, DP>( x_row, rows, f0, len, order, D, c, col );
	const int buf = mn_block_scan<DP>( col, s_el, D );
	// the replays are sequential, one lane each: the first MN_REPLAYS lanes of a wavefront take a team's each, and a wavefront left without one retires
	const int lane = threadIdx.x & 63, team = ( threadIdx.x >> 6 ) * MN_REPLAYS + lane;
	if( lane >= MN_REPLAYS || team >= TEAMS ) return;
	const int64_t r0 = ( block * TEAMS + team ) * run;
	const int r_len = int( std::min<int64_t>( std::max<int64_t>( n - r0, 0 ), run ) );
	if( r_len == 0 ) return;
	double in[DP];
	const double * cr = carry + int64_t( blockIdx.x ) * DP;
	#pragma unroll
	for( int i = 0; i < DP; ++i ) in[i] = cr[i];
	float s[DP];
	#pragma unroll
	for( int i = 0; i < DP; ++i ) s[i] = float( team == 0 ? in[i] : mn_apply<DP>( s_el[buf][team - 1], in, D, i ) );
	for( int i = 0; i < r_len; ++i )
		{
		const int64_t f = r0 + i;
		y_row[f] = mn_step32<KIND, DP>( x_row[f], rows.g[f], rows.R[f], rows.ik[f], rows.den[f], rows.mix[f], inv, order, s );
		}
	}

// ---- launcher -----------------------------------------------------------------------------------------------------------------------
struct MnArgs
	{
	const float * audio; int64_t ch, n; float sr;
	const float * cutoff; float cutoff_c;
	const float * damping; float damping_c;
	const float * feedback; float feedback_c;
	const float * wet_dry; float wet_dry_c;
	int kind, order, invert;
	float * out;
	};

// what both forms refuse before any device call
int mn_check( const MnArgs & a, MnLayout * l )
	{
	FLANHIP_REQUIRE( a.audio && a.out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( a.ch > 0 && a.n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( a.sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( a.kind == FLANHIP_MULTINOTCH_1POLE || a.kind == FLANHIP_MULTINOTCH_2POLE, FLANHIP_ERR_INVALID_ARG, "unknown multinotch kind" );
	FLANHIP_REQUIRE( a.order > 0, FLANHIP_ERR_INVALID_ARG, "order not positive" );
	FLANHIP_REQUIRE( mn_dim( a.kind, a.order ) <= MN_MAX_D, FLANHIP_ERR_UNSUPPORTED, "more than 16 states" );
	FLANHIP_REQUIRE( mn_layout( a.ch, a.n, a.kind, a.order, l ), FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

template<int KIND, int DP>
int mn_run( const MnArgs & a, const MnLayout & l, void * d_ws, hipStream_t s, volatile int * cancel )
	{
	auto go = [&]( auto kernel, int64_t blocks, auto... args ) { return launch_kernel( "launch_multinotch", kernel, blocks, MN_THREADS, 0, s, args... ); };
	const int64_t n = a.n, grid = l.blocks * a.ch;
	const float T_half = acosf( -1.0f ) / a.sr, nyquist = a.sr / 2.0f;        // :818
	const float inv = a.invert ? -1.0f : 1.0f;                                // :816
	double * den = ws_at<double>( d_ws, l.den ), * tot = ws_at<double>( d_ws, l.tot ), * carry = ws_at<double>( d_ws, l.carry );
	float * g = ws_at<float>( d_ws, l.g ), * R = ws_at<float>( d_ws, l.R ), * ik = ws_at<float>( d_ws, l.ik ), * mix = ws_at<float>( d_ws, l.mix );
	const MnRows rows{ den, g, R, ik, mix };
	if( int rc = go( k_mn_coef<KIND>, ( n + MN_THREADS - 1 ) / MN_THREADS, n, T_half, nyquist, a.cutoff, a.cutoff_c, a.damping, a.damping_c,
		a.feedback, a.feedback_c, a.wet_dry, a.wet_dry_c, inv, a.order, den, g, R, ik, mix ) ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	if( int rc = go( k_mn_sum<KIND, DP>, grid, a.audio, n, l.run, l.blocks, a.order, l.D, rows, tot ) ) return rc;
	if( int rc = go( k_mn_carry<DP>, a.ch, (const double*) tot, l.blocks, l.D, carry ) ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	return go( k_mn_replay<KIND, DP>, grid, a.audio, a.out, n, l.run, l.blocks, a.order, l.D, inv, rows, (const double*) carry );
	}

// cancel (the host form's flag, or null) is polled between the launches
int launch_multinotch( const MnArgs & a, void * d_ws, hipStream_t s, volatile int * cancel = nullptr )
	{
	MnLayout l;
	if( int rc = mn_check( a, &l ) ) return rc;
	FLANHIP_REQUIRE( d_ws, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	if( int rc = require_device() ) return rc;
	if( a.kind == FLANHIP_MULTINOTCH_1POLE )
		return l.DP == 4 ? mn_run<FLANHIP_MULTINOTCH_1POLE, 4>( a, l, d_ws, s, cancel )
			: l.DP == 8 ? mn_run<FLANHIP_MULTINOTCH_1POLE, 8>( a, l, d_ws, s, cancel )
			: mn_run<FLANHIP_MULTINOTCH_1POLE, 16>( a, l, d_ws, s, cancel );
	return l.DP == 4 ? mn_run<FLANHIP_MULTINOTCH_2POLE, 4>( a, l, d_ws, s, cancel )
		: l.DP == 8 ? mn_run<FLANHIP_MULTINOTCH_2POLE, 8>( a, l, d_ws, s, cancel )
		: mn_run<FLANHIP_MULTINOTCH_2POLE, 16>( a, l, d_ws, s, cancel );
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

size_t flanhip_multinotch_workspace_bytes( int64_t num_channels, int64_t num_frames, int kind, int order )
	{
	MnLayout l;
	if( !mn_layout( num_channels, num_frames, kind, order, &l ) ) return 0;
	return l.total;
	}

void flanhip_multinotch_debug_run( int frames )
	{
	t_mn_run = frames > 0 ? frames : 0;
	}

int flanhip_multinotch_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * d_cutoff, float cutoff, const float * d_damping, float damping, const float * d_feedback, float feedback,
	const float * d_wet_dry, float wet_dry, int kind, int order, int invert, float * d_out, void * d_workspace, void * stream )
	{
	const MnArgs a{ d_audio, num_channels, num_frames, sample_rate, d_cutoff, cutoff, d_damping, damping, d_feedback, feedback, d_wet_dry, wet_dry,
		kind, order, invert, d_out };
	return launch_multinotch( a, d_workspace, (hipStream_t) stream );
	}

int flanhip_multinotch( const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * cutoff_curve, float cutoff, const float * damping_curve, float damping, const float * feedback_curve, float feedback,
	const float * wet_dry_curve, float wet_dry, int kind, int order, int invert, float * out, volatile int * cancel )
	{
	MnArgs a{ audio, num_channels, num_frames, sample_rate, nullptr, cutoff, nullptr, damping, nullptr, feedback, nullptr, wet_dry, kind, order, invert, out };
	MnLayout l;
	if( int rc = mn_check( a, &l ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	const size_t x_bytes = sizeof( float ) * size_t( num_channels ) * size_t( num_frames ), row_bytes = sizeof( float ) * size_t( num_frames );
	HostCall call( cancel );
	void * d_ws = nullptr;
	if( int rc = call.in( audio, x_bytes, &a.audio ) ) return rc;
	if( int rc = call.out( out, x_bytes, &a.out ) ) return rc;
	if( int rc = call.scratch( l.total, &d_ws ) ) return rc;
	if( cutoff_curve ) if( int rc = call.in( cutoff_curve, row_bytes, &a.cutoff ) ) return rc;
	if( damping_curve && kind == FLANHIP_MULTINOTCH_2POLE ) if( int rc = call.in( damping_curve, row_bytes, &a.damping ) ) return rc;
	if( feedback_curve ) if( int rc = call.in( feedback_curve, row_bytes, &a.feedback ) ) return rc;
	if( wet_dry_curve ) if( int rc = call.in( wet_dry_curve, row_bytes, &a.wet_dry ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_multinotch( a, d_ws, nullptr, cancel ) ) return rc;
	return call.finish();
	}

} // extern "C"
