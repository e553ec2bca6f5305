// halfband.hip -- hilbert_phase_diff_network (Audio/AudioFilter.cpp:1045-1160) and what rests on it: Audio::halfband_modulate (:1162-1186),
// the modulation stage of Audio::shift_frequency (:1188-1227) and Audio::halfband_multiply (:1229-1263).  DESIGN.md section 4.17.
//
// The network is two cascades of K = 10 one-pole all-pass sections (:61-80 with the mix { 1, -1 } and no prewarp) whose poles are constants
// (:1109-1150).  A section is linear in its state, and its coefficient G = g / ( 1 + g ) is the same at every frame:
//   s' = ( 1 - 2 G ) s + 2 G x,        y = 2 ( 1 - G ) s + ( 2 G - 1 ) x            (y is the next section's x)
// so a whole cascade is ONE linear system s' = A s + b x with s in R^K and a constant lower-triangular A.  A run of L frames from the state
// s is A^L s + r, r the run's response from the state 0: every map a scan over the frames composes is a power of the same A, and the scan
// element is the vector r alone.  Every lane's run counts as `run` frames (frames past n are zero input), so the power that goes with a span
// of lanes is one of a small table, P_k = A^( run 2^k ), k = 0 ... 14, which k_hb_table builds in fp64 by repeated squaring, on the stream.
//   k_hb_sum         every lane runs the cascades over its run from 0 in fp64 (the sections one after the other: 4 operations a section),
//                    the wavefront scans the responses (Hillis-Steele: at offset 2^k the receiving lane's partial covers 2^k lanes, so
//                    the step is P_k shuffled + mine), the four wavefront totals combine with P_6 into the block's total
//   k_hb_carry       one block per channel and cascade: the same scan over the block totals with P_8 ... P_13, 64 totals a wavefront (P_14
//                    between wavefronts), from the state 0 before frame 0: the state at every block's first frame
//   k_hb_replay      scans the block again, advances the state that enters the wavefront to every lane by the binary digits of the lane
//                    (P_0 ... P_5; powers of A commute), rounds the lane's start state to fp32 ONCE and replays the run with the
//                    reference's own fp32 operations in the reference's order (filter.hip's rule).  What happens to the cascades' outputs is
//                    the template parameter EPI; in the fused forms they never go to memory.
// Four launches whatever K is; both cascades of a network -- with two operands (halfband_multiply) all four -- share them.  No block waits
// for another, no flags, no atomics; every composition runs in a fixed order: two calls agree bit for bit and a channel does not depend
// on the channels beside it.  A lane reads its run before it writes it and reads no other lane's: an output may be an input.
// Nothing is truncated: the scan is exact for any run length and sample rate, however far the network's memory reaches.
#include "run_scan.h"

namespace flanhip {

namespace {

thread_local int t_hb_run = 0;            // flanhip_halfband_debug_run: frames per lane forced for the calling thread (0: the library's choice)

constexpr int HB_K = 10;                              // sections of one cascade
constexpr int HB_TRI = HB_K * ( HB_K + 1 ) / 2;       // a lower-triangular matrix, packed by rows: ( i, j ) at i ( i + 1 ) / 2 + j
constexpr int HB_POWERS = 15;                         // P_0 ... P_5 lanes of a wavefront, P_6 ... P_7 wavefronts, P_8 ... P_14 blocks
constexpr int HB_MAX_CASCADES = 4;                    // two operands of two cascades each
constexpr int HB_TABLE_THREADS = 128;
constexpr int HB_CARRY_THREADS = 1024;                // sixteen wavefronts: 1024 block totals a pass
constexpr int64_t HB_MAX_FRAMES = int64_t( 1 ) << 36;
constexpr int64_t HB_MAX_CHANNELS = 1 << 20;
constexpr int64_t HB_MAX_GRID = ( int64_t( 1 ) << 31 ) - 1;      // blocks x channels of one launch

struct HbLayout
	{
	int run = 0;
	int64_t blocks = 0;                   // per channel
	size_t table = 0, tot = 0, carry = 0, total = 0;
	};

// the workspace: the tables of four cascades, then per channel and block the four cascades' totals and carried states (sized for
// halfband_multiply whatever the call)
bool hb_layout( int64_t ch, int64_t n, HbLayout * l )
	{
	if( ch <= 0 || n <= 0 || ch > HB_MAX_CHANNELS || n > HB_MAX_FRAMES ) return false;
	l->run = scan_run( t_hb_run );
	l->blocks = scan_blocks( n, l->run );
	if( l->blocks > HB_MAX_GRID / ch ) return false;
	const size_t units = size_t( ch ) * size_t( l->blocks ), unit = sizeof( double ) * HB_MAX_CASCADES * HB_K;
	l->table = 0;
	l->tot = sizeof( double ) * HB_MAX_CASCADES * HB_POWERS * HB_TRI;
	l->carry = l->tot + unit * units;
	l->total = l->carry + unit * units;
	return true;
	}

// ---- the poles (:1109-1150), in fp64 as the reference computes them, each rounded to fp32 -------------------------------------------------
void hb_poles( float first[HB_K], float second[HB_K] )
	{
	const double pi = 3.14159265358979323846;               // std::_Pi
	const float f_l = 5.0f, f_u = 22000.0f;                 // :1156
	const double B = f_u / f_l;
	const double k = std::sqrt( 1.0 - 1.0 / ( B * B ) );
	const double L = 0.5 * ( 1.0 - std::sqrt( k ) ) / ( 1.0 + std::sqrt( k ) );
	const double A_p = L + 2.0 * std::pow( L, 5.0 ) + 15.0 * std::pow( L, 9.0 );
	const double A = std::exp( pi * pi / std::log( A_p ) );
	const double n = 2 * HB_K;
	for( int r = 0; r < 2 * HB_K; ++r )
		{
		const double phi = pi / 4.0 / n * ( 2 * ( r + 1 ) - 1 );
		const double numerator = ( A * A - A * A * A * A * A * A ) * std::sin( 4.0 * phi );
		const double denominator = 1.0 + ( A * A + A * A * A * A * A * A ) * std::cos( 4.0 * phi );
		const double phi_p = std::atan( numerator / denominator );
		const float p = float( std::sqrt( B ) * std::tan( phi - phi_p ) * 2.0 * pi * f_l );
		// :1143-1149: the even indices are p_a, the odd ones p_b, and ( p_b, p_a ) goes back: the FIRST cascade has the odd-indexed poles
		( r % 2 ? first : second )[r / 2] = p;
		}
	}

// What the kernels are told of NC cascades: G in fp32 as the replay uses it, 2 G in fp64 for the maps
template<int NC>
struct HbCoef
	{
	float G[NC][HB_K];
	double G2[NC][HB_K];
	};

// :57, :67-68 with the pole as w (no prewarp, no clamp): T_half = pi / sr, g = p T_half, G = g / ( 1 + g ), in fp32
void hb_coef( float sr, float ( &G )[HB_K], double ( &G2 )[HB_K], const float ( &poles )[HB_K] )
	{
	const float T_half = acosf( -1.0f ) / sr;
	for( int i = 0; i < HB_K; ++i )
		{
		const float g = poles[i] * T_half;
		G[i] = g / ( 1.0f + g );
		G2[i] = 2.0 * double( G[i] );
		}
	}

// ---- one frame through a cascade ------------------------------------------------------------------------------------------------------
// in fp32, the reference's operations in its order, one rounding each (:69-71, :79): the cascade's output
__device__ __forceinline__ float hb_step32( const float ( &G )[HB_K], float ( &s )[HB_K], float x )
	{
	#pragma unroll
	for( int i = 0; i < HB_K; ++i )
		{
		const float v = G[i] * ( x - s[i] );
		const float lp = v + s[i];
		s[i] = lp + v;
		x = lp - ( x - lp );                        // lp * 1 + ( x - lp ) * -1: the products are exact
		}
	return x;
	}
// the same frame as a map of the state, in fp64 from the fp32 G: s' = s + 2 G ( x - s ), y = 2 lp - x = ( s + s' ) - x
__device__ __forceinline__ void hb_step64( const double ( &G2 )[HB_K], double ( &s )[HB_K], double x )
	{
	#pragma unroll
	for( int i = 0; i < HB_K; ++i )
		{
		const double next = fma( G2[i], x - s[i], s[i] );
		x = ( s[i] + next ) - x;
		s[i] = next;
		}
	}

// v = P v, P lower triangular and the same for every lane (from the highest row down, so in place)
__device__ __forceinline__ void hb_mul( const double * __restrict__ P, double ( &v )[HB_K] )
	{
	#pragma unroll
	for( int i = HB_K - 1; i >= 0; --i )
		{
		double acc = P[i * ( i + 1 ) / 2] * v[0];
		#pragma unroll
		for( int j = 1; j <= i; ++j ) acc = fma( P[i * ( i + 1 ) / 2 + j], v[j], acc );
		v[i] = acc;
		}
	}
// the power k of cascade c
__device__ __forceinline__ const double * hb_power( const double * __restrict__ table, int c, int k ) { return table + ( c * HB_POWERS + k ) * HB_TRI; }

// The scan of one response per lane over the wavefront, in lane order, with the powers first ... first + 5: `inc` becomes the response of
// the lanes 0 ... lane together (each lane's span counted as the span of `first`)
__device__ __forceinline__ void hb_wave_scan( const double * __restrict__ table, int c, int first, double ( &inc )[HB_K] )
	{
	const int lane = threadIdx.x & 63;
	#pragma unroll
	for( int k = 0; k < 6; ++k )
		{
		double o[HB_K];
		#pragma unroll
		for( int i = 0; i < HB_K; ++i ) o[i] = __shfl_up( inc[i], 1 << k );
		hb_mul( hb_power( table, c, first + k ), o );
		if( lane >= ( 1 << k ) )
			{
			#pragma unroll
			for( int i = 0; i < HB_K; ++i ) inc[i] += o[i];
			}
		}
	}
// the state `s` that enters lane 0 moved on to the calling lane: through `lane` spans of the power `first`
__device__ __forceinline__ void hb_advance( const double * __restrict__ table, int c, int first, double ( &s )[HB_K] )
	{
	const int lane = threadIdx.x & 63;
	#pragma unroll
	for( int k = 0; k < 6; ++k )
		if( lane >> k & 1 ) hb_mul( hb_power( table, c, first + k ), s );
	}

// ---- kernels ----------------------------------------------------------------------------------------------------------------------
// One block per cascade: A from one step of every unit state, P_0 = A^run by binary powers, then fourteen squarings; the lower triangles
// go to the table.  All in fp64, in LDS, one thread per entry.
template<int NC>
__global__ __launch_bounds__( HB_TABLE_THREADS ) void k_hb_table( HbCoef<NC> coef, int run, double * __restrict__ table )
	{
	__shared__ double R[HB_K * HB_K], B[HB_K * HB_K];
	const int c = blockIdx.x, t = threadIdx.x, i = t / HB_K, j = t % HB_K;
	const bool on = t < HB_K * HB_K;
	if( t < HB_K )
		{
		double G2[HB_K], s[HB_K];
		#pragma unroll
		for( int m = 0; m < HB_K; ++m ) { G2[m] = 0.0; s[m] = m == t ? 1.0 : 0.0; }
		#pragma unroll
		for( int cc = 0; cc < NC; ++cc )
			if( cc == c )
				{
				#pragma unroll
				for( int m = 0; m < HB_K; ++m ) G2[m] = coef.G2[cc][m];
				}
		hb_step64( G2, s, 0.0 );
		#pragma unroll
		for( int m = 0; m < HB_K; ++m ) B[m * HB_K + t] = s[m];              // column t of A
		}
	if( on ) R[t] = i == j ? 1.0 : 0.0;
	__syncthreads();
	// Z = X Y; Z may be X or Y
	auto mul = [&]( const double * X, const double * Y, double * Z )
		{
		double acc = 0.0;
		if( on ) for( int m = 0; m < HB_K; ++m ) acc = fma( X[i * HB_K + m], Y[m * HB_K + j], acc );
		__syncthreads();
		if( on ) Z[t] = acc;
		__syncthreads();
		};
	for( int e = run; e > 0; )
		{
		if( e & 1 ) mul( B, R, R );
		e >>= 1;
		if( e ) mul( B, B, B );
		}
	for( int k = 0; k < HB_POWERS; ++k )
		{
		if( on && j <= i ) table[( c * HB_POWERS + k ) * HB_TRI + i * ( i + 1 ) / 2 + j] = R[t];
		mul( R, R, R );
		}
	}

// The rows of the operands: cascades 2 o and 2 o + 1 read operand o
struct HbIn { const float * p; int64_t stride; };
template<int NC>
struct HbScan
	{
	HbIn in[NC / 2];
	int64_t n; int run; int64_t blocks;
	const double * table;
	};

// every cascade's response to the lane's run from the state 0, the run counted as `run` frames
template<int NC, bool VEC>
__device__ __forceinline__ void hb_summarise( const HbScan<NC> & a, const HbCoef<NC> & coef, int64_t channel, int64_t f0, int len, double ( &r )[NC][HB_K] )
	{
	#pragma unroll
	for( int c = 0; c < NC; ++c )
		{
		#pragma unroll
		for( int i = 0; i < HB_K; ++i ) r[c][i] = 0.0;
		}
	if( len == 0 ) return;
	for( int i = 0; i < a.run; i += 4 )
		{
		#pragma unroll
		for( int o = 0; o < NC / 2; ++o )
			{
			float x[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
			if( i < len ) load4<VEC>( a.in[o].p + channel * a.in[o].stride, f0 + i, len - i, x );
			#pragma unroll
			for( int k = 0; k < 4; ++k )
				if( i + k < a.run )
					{
					hb_step64( coef.G2[2 * o], r[2 * o], double( x[k] ) );
					hb_step64( coef.G2[2 * o + 1], r[2 * o + 1], double( x[k] ) );
					}
			}
		}
	}

// tot: [channels x blocks][NC][HB_K]
template<int NC, bool VEC>
__global__ __launch_bounds__( SCAN_THREADS ) void k_hb_sum( HbScan<NC> a, HbCoef<NC> coef, double * __restrict__ tot )
	{
	__shared__ double s_tot[SCAN_WAVES][NC][HB_K];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int64_t channel, f0; int len;
	lane_run( a.n, a.run, a.blocks, channel, f0, len );
	double r[NC][HB_K];
	hb_summarise<NC, VEC>( a, coef, channel, f0, len, r );
	#pragma unroll
	for( int c = 0; c < NC; ++c )
		{
		hb_wave_scan( a.table, c, 0, r[c] );
		if( lane == 63 )
			{
			#pragma unroll
			for( int i = 0; i < HB_K; ++i ) s_tot[wave][c][i] = r[c][i];
			}
		}
	__syncthreads();
	// thread c: cascade c's total, the wavefronts' in order
	if( threadIdx.x < NC )
		{
		const int c = threadIdx.x;
		double total[HB_K];
		#pragma unroll
		for( int i = 0; i < HB_K; ++i ) total[i] = s_tot[0][c][i];
		for( int w = 1; w < SCAN_WAVES; ++w )
			{
			hb_mul( hb_power( a.table, c, 6 ), total );
			#pragma unroll
			for( int i = 0; i < HB_K; ++i ) total[i] += s_tot[w][c][i];
			}
		#pragma unroll
		for( int i = 0; i < HB_K; ++i ) tot[( int64_t( blockIdx.x ) * NC + c ) * HB_K + i] = total[i];
		}
	}

// One block per channel and cascade: the state at the first frame of every block of the scan, from the block totals and the state 0 before
// frame 0.  Every wavefront scans 64 totals; thread 0 takes the state through the wavefronts' totals in order (P_14 each); every
// wavefront then advances the state that enters it to its lanes.  More than 1024 blocks a channel: the same again from the state left
template<int NC>
__global__ __launch_bounds__( HB_CARRY_THREADS ) void k_hb_carry( const double * __restrict__ tot, int64_t blocks, const double * __restrict__ table, double * __restrict__ carry )
	{
	constexpr int WAVES = HB_CARRY_THREADS / 64;
	__shared__ double s_tot[WAVES][HB_K], s_enter[WAVES + 1][HB_K];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t channel = int64_t( blockIdx.x ) / NC;
	const int c = int( int64_t( blockIdx.x ) - channel * NC );
	for( int64_t base = 0; base < blocks; base += HB_CARRY_THREADS )
		{
		const int64_t b = base + threadIdx.x;
		const int64_t at = ( ( channel * blocks + b ) * NC + c ) * HB_K;
		double inc[HB_K], start[HB_K];
		#pragma unroll
		for( int i = 0; i < HB_K; ++i ) inc[i] = b < blocks ? tot[at + i] : 0.0;
		hb_wave_scan( table, c, 8, inc );
		if( lane == 63 )
			{
			#pragma unroll
			for( int i = 0; i < HB_K; ++i ) s_tot[wave][i] = inc[i];
			}
		__syncthreads();
		if( threadIdx.x == 0 )
			{
			double state[HB_K];
			#pragma unroll
			for( int i = 0; i < HB_K; ++i ) state[i] = base == 0 ? 0.0 : s_enter[WAVES][i];
			for( int w = 0; w < WAVES; ++w )
				{
				#pragma unroll
				for( int i = 0; i < HB_K; ++i ) s_enter[w][i] = state[i];
				hb_mul( hb_power( table, c, 14 ), state );
				#pragma unroll
				for( int i = 0; i < HB_K; ++i ) state[i] += s_tot[w][i];
				}
			#pragma unroll
			for( int i = 0; i < HB_K; ++i ) s_enter[WAVES][i] = state[i];
			}
		__syncthreads();
		#pragma unroll
		for( int i = 0; i < HB_K; ++i ) start[i] = s_enter[wave][i];
		hb_advance( table, c, 8, start );
		#pragma unroll
		for( int i = 0; i < HB_K; ++i )
			{
			const double before = __shfl_up( inc[i], 1 );
			if( lane > 0 ) start[i] += before;
			}
		if( b < blocks )
			{
			#pragma unroll
			for( int i = 0; i < HB_K; ++i ) carry[at + i] = start[i];
			}
		}
	}

// What becomes of the cascades' outputs y_0 ... of a frame (each product and the difference one fp32 rounding, no fused multiply-add):
//   EPI_BOTH       out = y_0, out2 = y_1                                           (hilbert_phase_diff_network)
//   EPI_ROWS       out = y_0 re[f] - y_1 im[f], each a row or (null) the scalar       (:1178-1181)
//   EPI_PHASE      the same with re = cos( phase[f] ), im = sin( phase[f] ): the fp64 functions of the fp32 phase rounded to fp32 once (:1225)
//   EPI_PRODUCT    out = y_0 y_2 - y_1 y_3, four cascades over two operands           (:1254-1258)
enum { EPI_BOTH, EPI_ROWS, EPI_PHASE, EPI_PRODUCT };
struct HbOut
	{
	float * out, * out2;
	const float * re, * im, * phase;
	float re_c, im_c;
	};

// out and out2: rows of n frames.  Either may be an operand: a lane has read its quad when it writes it, and reads no other lane's run
template<int NC, bool VEC, int EPI>
__global__ __launch_bounds__( SCAN_THREADS ) void k_hb_replay( HbScan<NC> a, HbCoef<NC> coef, const double * __restrict__ carry, HbOut e )
	{
	__shared__ double s_tot[SCAN_WAVES][NC][HB_K];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int64_t channel, f0; int len;
	lane_run( a.n, a.run, a.blocks, channel, f0, len );
	double r[NC][HB_K];
	hb_summarise<NC, VEC>( a, coef, channel, f0, len, r );
	#pragma unroll
	for( int c = 0; c < NC; ++c )
		{
		hb_wave_scan( a.table, c, 0, r[c] );
		if( lane == 63 )
			{
			#pragma unroll
			for( int i = 0; i < HB_K; ++i ) s_tot[wave][c][i] = r[c][i];
			}
		}
	__syncthreads();
	float s[NC][HB_K];
	#pragma unroll
	for( int c = 0; c < NC; ++c )
		{
		// the state that enters the wavefront: the block's carried one through the wavefronts before this one
		double start[HB_K];
		#pragma unroll
		for( int i = 0; i < HB_K; ++i ) start[i] = carry[( int64_t( blockIdx.x ) * NC + c ) * HB_K + i];
		for( int w = 0; w < wave; ++w )
			{
			hb_mul( hb_power( a.table, c, 6 ), start );
			#pragma unroll
			for( int i = 0; i < HB_K; ++i ) start[i] += s_tot[w][c][i];
			}
		hb_advance( a.table, c, 0, start );
		#pragma unroll
		for( int i = 0; i < HB_K; ++i )
			{
			const double before = __shfl_up( r[c][i], 1 );
			if( lane > 0 ) start[i] += before;
			s[c][i] = float( start[i] );
			}
		}
	float * out_row = e.out + channel * a.n;
	for( int i = 0; i < len; i += 4 )
		{
		float x[NC / 2][4], y[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, y2[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
		float re[4] = { e.re_c, e.re_c, e.re_c, e.re_c }, im[4] = { e.im_c, e.im_c, e.im_c, e.im_c };
		#pragma unroll
		for( int o = 0; o < NC / 2; ++o ) load4<VEC>( a.in[o].p + channel * a.in[o].stride, f0 + i, len - i, x[o] );
		if constexpr( EPI == EPI_ROWS )
			{
			if( e.re ) load4<VEC>( e.re, f0 + i, len - i, re );
			if( e.im ) load4<VEC>( e.im, f0 + i, len - i, im );
			}
		if constexpr( EPI == EPI_PHASE )
			{
			float phase[4];
			load4<VEC>( e.phase, f0 + i, len - i, phase );
			#pragma unroll
			for( int k = 0; k < 4; ++k )
				{
				re[k] = float( cos( double( phase[k] ) ) );
				im[k] = float( sin( double( phase[k] ) ) );
				}
			}
		#pragma unroll
		for( int k = 0; k < 4; ++k )
			if( i + k < len )
				{
				float v[NC];
				#pragma unroll
				for( int c = 0; c < NC; ++c ) v[c] = hb_step32( coef.G[c], s[c], x[c / 2][k] );
				if constexpr( EPI == EPI_BOTH ) { y[k] = v[0]; y2[k] = v[1]; }
				else if constexpr( EPI == EPI_PRODUCT )
					{
					const float p = v[0] * v[NC - 2], q = v[1] * v[NC - 1];
					y[k] = p - q;
					}
				else
					{
					const float p = v[0] * re[k], q = v[1] * im[k];
					y[k] = p - q;
					}
				}
		store4<VEC>( out_row, f0 + i, len - i, y );
		if constexpr( EPI == EPI_BOTH ) store4<VEC>( e.out2 + channel * a.n, f0 + i, len - i, y2 );
		}
	}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
struct HbOperand { const float * p; int64_t ch, n; float sr; };

int hb_check_operand( const HbOperand & x )
	{
	FLANHIP_REQUIRE( x.p, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( x.ch > 0 && x.n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( x.sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	return FLANHIP_OK;
	}

// what both forms of an entry point refuse before any device call; ch and n: the output's
int hb_check( const HbOperand * ops, int count, const HbOut & e, int epi, int64_t ch, int64_t n, HbLayout * l )
	{
	FLANHIP_REQUIRE( e.out && ( epi != EPI_BOTH || e.out2 ), FLANHIP_ERR_INVALID_ARG, "null buffer" );
	for( int o = 0; o < count; ++o ) if( int rc = hb_check_operand( ops[o] ) ) return rc;
	FLANHIP_REQUIRE( hb_layout( ch, n, l ), FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

// the network over one operand (NC = 2) or two (NC = 4): the table, the totals, the carries, the replay with its epilogue
template<int NC, int EPI>
int launch_halfband( const HbOperand * ops, int64_t ch, int64_t n, const HbOut & e, void * d_ws, hipStream_t s )
	{
	HbLayout l;
	if( int rc = hb_check( ops, NC / 2, e, EPI, ch, n, &l ) ) return rc;
	FLANHIP_REQUIRE( d_ws, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	if( int rc = require_device() ) return rc;
	float first[HB_K], second[HB_K];
	hb_poles( first, second );
	HbCoef<NC> coef;
	HbScan<NC> a;
	double * table = ws_at<double>( d_ws, l.table ), * tot = ws_at<double>( d_ws, l.tot ), * carry = ws_at<double>( d_ws, l.carry );
	a.n = n; a.run = l.run; a.blocks = l.blocks; a.table = table;
	// 16-byte loads and stores: every run and every row of every buffer then starts on a 16-byte boundary and ends on a whole quad
	bool vec = l.run % 4 == 0 && n % 4 == 0 && aligned16( e.out ) && aligned16( e.out2 ) && aligned16( e.re ) && aligned16( e.im ) && aligned16( e.phase );
	for( int o = 0; o < NC / 2; ++o )
		{
		hb_coef( ops[o].sr, coef.G[2 * o], coef.G2[2 * o], first );
		hb_coef( ops[o].sr, coef.G[2 * o + 1], coef.G2[2 * o + 1], second );
		a.in[o] = HbIn{ ops[o].p, ops[o].n };
		vec = vec && ops[o].n % 4 == 0 && aligned16( ops[o].p );
		}
	const int64_t grid = l.blocks * ch;
	auto go = [&]( auto kernel, int64_t blocks, int threads, auto... args ) { return launch_kernel( "launch_halfband", kernel, blocks, threads, 0, s, args... ); };
	if( int rc = go( k_hb_table<NC>, NC, HB_TABLE_THREADS, coef, l.run, table ) ) return rc;
	if( int rc = scan_pair( vec, [&]( auto V ) { return go( k_hb_sum<NC, V.value>, grid, SCAN_THREADS, a, coef, tot ); } ) ) return rc;
	if( int rc = go( k_hb_carry<NC>, ch * NC, HB_CARRY_THREADS, (const double*) tot, l.blocks, (const double*) table, carry ) ) return rc;
	return scan_pair( vec, [&]( auto V ) { return go( k_hb_replay<NC, V.value, EPI>, grid, SCAN_THREADS, a, coef, (const double*) carry, e ); } );
	}

int launch_modulate( const HbOperand & x, const HbOut & e, void * d_ws, hipStream_t s )
	{
	if( e.phase ) return launch_halfband<2, EPI_PHASE>( &x, x.ch, x.n, e, d_ws, s );
	return launch_halfband<2, EPI_ROWS>( &x, x.ch, x.n, e, d_ws, s );
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

void flanhip_halfband_poles( float first[10], float second[10] )
	{
	hb_poles( first, second );
	}

size_t flanhip_halfband_workspace_bytes( int64_t num_channels, int64_t num_frames )
	{
	HbLayout l;
	if( !hb_layout( num_channels, num_frames, &l ) ) return 0;
	return l.total;
	}

void flanhip_halfband_debug_run( int frames )
	{
	t_hb_run = frames > 0 ? frames : 0;
	}

int flanhip_hilbert_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	float * d_first, float * d_second, void * d_workspace, void * stream )
	{
	const HbOperand x{ d_audio, num_channels, num_frames, sample_rate };
	const HbOut e{ d_first, d_second, nullptr, nullptr, nullptr, 0.0f, 0.0f };
	return launch_halfband<2, EPI_BOTH>( &x, num_channels, num_frames, e, d_workspace, (hipStream_t) stream );
	}

int flanhip_hilbert( const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	float * first, float * second, volatile int * cancel )
	{
	HbOperand x{ audio, num_channels, num_frames, sample_rate };
	HbOut e{ first, second, nullptr, nullptr, nullptr, 0.0f, 0.0f };
	HbLayout l;
	if( int rc = hb_check( &x, 1, e, EPI_BOTH, num_channels, num_frames, &l ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	const size_t x_bytes = sizeof( float ) * size_t( num_channels ) * size_t( num_frames );
	HostCall call( cancel );
	void * d_ws = nullptr;
	if( int rc = call.in( audio, x_bytes, &x.p ) ) return rc;
	if( int rc = call.out( first, x_bytes, &e.out ) ) return rc;
	if( int rc = call.out( second, x_bytes, &e.out2 ) ) return rc;
	if( int rc = call.scratch( l.total, &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_halfband<2, EPI_BOTH>( &x, num_channels, num_frames, e, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

int flanhip_halfband_modulate_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * d_re, float re, const float * d_im, float im, const float * d_phase, float * d_out, void * d_workspace, void * stream )
	{
	const HbOperand x{ d_audio, num_channels, num_frames, sample_rate };
	const HbOut e{ d_out, nullptr, d_phase ? nullptr : d_re, d_phase ? nullptr : d_im, d_phase, re, im };
	return launch_modulate( x, e, d_workspace, (hipStream_t) stream );
	}

int flanhip_halfband_modulate( const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * re_curve, float re, const float * im_curve, float im, const float * phase_curve, float * out, volatile int * cancel )
	{
	HbOperand x{ audio, num_channels, num_frames, sample_rate };
	HbOut e{ out, nullptr, nullptr, nullptr, nullptr, re, im };
	HbLayout l;
	if( int rc = hb_check( &x, 1, e, EPI_ROWS, num_channels, num_frames, &l ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	const size_t x_bytes = sizeof( float ) * size_t( num_channels ) * size_t( num_frames ), row_bytes = sizeof( float ) * size_t( num_frames );
	HostCall call( cancel );
	void * d_ws = nullptr;
	if( int rc = call.in( audio, x_bytes, &x.p ) ) return rc;
	if( int rc = call.out( out, x_bytes, &e.out ) ) return rc;
	if( int rc = call.scratch( l.total, &d_ws ) ) return rc;
	if( phase_curve ) { if( int rc = call.in( phase_curve, row_bytes, &e.phase ) ) return rc; }
	else
		{
		if( re_curve ) if( int rc = call.in( re_curve, row_bytes, &e.re ) ) return rc;
		if( im_curve ) if( int rc = call.in( im_curve, row_bytes, &e.im ) ) return rc;
		}
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_modulate( x, e, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

int flanhip_halfband_multiply_dev( const float * d_a, int64_t channels_a, int64_t frames_a, float sample_rate_a,
	const float * d_b, int64_t channels_b, int64_t frames_b, float sample_rate_b, float * d_out, void * d_workspace, void * stream )
	{
	const HbOperand ops[2] = { { d_a, channels_a, frames_a, sample_rate_a }, { d_b, channels_b, frames_b, sample_rate_b } };
	const HbOut e{ d_out, nullptr, nullptr, nullptr, nullptr, 0.0f, 0.0f };
	return launch_halfband<4, EPI_PRODUCT>( ops, std::min( channels_a, channels_b ), std::min( frames_a, frames_b ), e, d_workspace, (hipStream_t) stream );
	}

int flanhip_halfband_multiply( const float * a, int64_t channels_a, int64_t frames_a, float sample_rate_a,
	const float * b, int64_t channels_b, int64_t frames_b, float sample_rate_b, float * out, volatile int * cancel )
	{
	HbOperand ops[2] = { { a, channels_a, frames_a, sample_rate_a }, { b, channels_b, frames_b, sample_rate_b } };
	HbOut e{ out, nullptr, nullptr, nullptr, nullptr, 0.0f, 0.0f };
	const int64_t ch = std::min( channels_a, channels_b ), n = std::min( frames_a, frames_b );
	HbLayout l;
	if( int rc = hb_check( ops, 2, e, EPI_PRODUCT, ch, n, &l ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	void * d_ws = nullptr;
	for( HbOperand & x : ops ) if( int rc = call.in( x.p, sizeof( float ) * size_t( x.ch ) * size_t( x.n ), &x.p ) ) return rc;
	if( int rc = call.out( out, sizeof( float ) * size_t( ch ) * size_t( n ), &e.out ) ) return rc;
	if( int rc = call.scratch( l.total, &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_halfband<4, EPI_PRODUCT>( ops, ch, n, e, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

} // extern "C"
