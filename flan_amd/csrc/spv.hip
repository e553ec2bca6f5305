// spv.hip -- the sliding-DFT phase vocoder: Audio::convert_to_SPV / SPV::convert_to_audio (Conversions/AudioSPV.cpp) and the
// constant forms of SPV::modify_frequency / repitch (SPV/SPV.cpp).  DESIGN.md section 4.11.
//
// Analysis.  The reference's running sum S[f][b] = S[f-1][b] + d[f] T[(f b) mod L] over d[f] = x[f] - x[f-L] (AudioSPV.cpp:45-58)
// telescopes: S[f][b] = sum_{f-L < j <= f} x[j] T[(j b) mod L], the L-point DFT of the window that ends at f, times T[(f+1) b].  So a
// chain of frames [f0, f0 + C) needs no predecessor: it seeds S at frame f0 - 2 with that direct sum over the L samples before it, then
// walks the reference's additive step (same fp32 operations, same order) through a halo frame f0 - 1 (its phase is `prev` of frame f0)
// and its own frames.  A wavefront owns one chain and one tile of 64 B contiguous bins (B per lane); the Hann 3-tap needs the neighbour
// lanes' demodulated values (shuffles) and, at the tile's two ends, one extra bin that lanes 0 and 63 walk alongside their own.
//
// Synthesis.  Per bin the reference accumulates phase increments in fp64 and folds them (phase_vocoder.cpp:55-61); a chain of frames
// starts from its carry: k_spv_chain_sums sums every chain (its total and its highest prefix sum), k_spv_scan turns them into the
// phases the reference holds at the chains' starts, and k_spv_synthesize walks each chain from its carry, one block per chain, and
// reduces the bins of 32 frames at a time through LDS.
//
// All indices are 64-bit: the reference's int32 (f b) % L turns negative past f b >= 2^31 (AudioSPV.cpp:38), here the twiddle index is
// (f b) mod L as intended.  num_bins < 2 is refused (the reference reads bin 1 of a one-bin frame, AudioSPV.cpp:67).
#include "flanhip_internal.h"
#include "pv_math.h"

#include <algorithm>
#include <complex>

namespace flanhip {

namespace {

thread_local int t_spv_chain_len = 0;     // flanhip_spv_debug_chain_length: frames per chain (0: the library's choice)

constexpr int SPV_SYN_THREADS = 256;      // synthesis block
constexpr int SPV_SYN_FB = 32;            // frames reduced per batch
constexpr int SPV_XB = 64;                // analysis: samples staged in LDS per batch (one per lane)

// The twiddle table of one transform length L = 2 num_bins (AudioSPV.cpp:13-22, :37): T[i] = polar( 1.0f, omega i ) with the float
// omega = -pi2 / L, evaluated on the host with the same float expression so that the table is the reference's to the bit.
struct SpvTable { float2 * d = nullptr; };
std::mutex g_spv_mutex;
std::map<std::pair<int, int>, SpvTable> g_spv_tables;      // (device, L) -> table

void host_twiddles( int L, float * out2 )
	{
	const float pi2 = 6.2831854820251465f;
	const float omega = -pi2 / float( L );
	for( int i = 0; i < L; ++i )
		{
		const std::complex<float> t = std::polar( 1.0f, omega * float( i ) );
		out2[2 * i] = t.real();
		out2[2 * i + 1] = t.imag();
		}
	}

int get_table( int L, const float2 ** out )
	{
	int dev = 0;
	FLANHIP_CHECK( hipGetDevice( &dev ) );
	std::lock_guard<std::mutex> lock( g_spv_mutex );
	SpvTable & t = g_spv_tables[{ dev, L }];
	if( !t.d )
		{
		std::vector<float> h( 2 * size_t( L ) );
		host_twiddles( L, h.data() );
		float2 * d = nullptr;
		FLANHIP_CHECK( hipMalloc( &d, sizeof( float2 ) * size_t( L ) ) );
		if( hipMemcpy( d, h.data(), sizeof( float2 ) * size_t( L ), hipMemcpyHostToDevice ) != hipSuccess )
			{
			(void) hipFree( d );
			set_error( "spv twiddle upload failed" );
			return FLANHIP_ERR_HIP;
			}
		t.d = d;
		}
	*out = t.d;
	return FLANHIP_OK;
	}

// bins per lane of the analysis: 8 from 512 bins up (a tile of 512 bins per wavefront), fewer below so that a small transform still
// spreads over the wavefront
int spv_bins_per_lane( int N )
	{
	int B = 1;
	while( B < 8 && 64 * B < N ) B *= 2;
	return B;
	}

// The analysis cut.  A chain of C frames pays a seed of L frames of ~6 instructions per bin against ~70 per emitted frame: C >= 0.35 L
// keeps the seed at <= 25 % of the chain.  Above that, chains grow until the launch fills 8 wavefronts per CU once.
int64_t spv_analysis_chain( int64_t ch, int64_t n, int N, int tiles )
	{
	if( t_spv_chain_len > 0 ) return t_spv_chain_len;
	const int64_t L = 2 * int64_t( N );
	const int64_t c_seed = std::max<int64_t>( 16, ( 35 * L + 99 ) / 100 );
	const int64_t slots = int64_t( cu_count() ) * 8;
	const int64_t c_fill = ( ch * tiles * n + slots - 1 ) / slots;
	return std::max<int64_t>( 1, std::min<int64_t>( std::max( c_seed, c_fill ), std::max<int64_t>( n, 1 ) ) );
	}

// The synthesis cut: pure host arithmetic (the workspace is sized from it without a device).  Whole batches of 32 frames, and about
// 2048 blocks over the launch.
int64_t spv_synthesis_chain( int64_t ch, int64_t n )
	{
	if( t_spv_chain_len > 0 ) return t_spv_chain_len;
	int64_t c = ( ch * n + 2047 ) / 2048;
	c = ( ( c + SPV_SYN_FB - 1 ) / SPV_SYN_FB ) * SPV_SYN_FB;
	return std::max<int64_t>( 4 * SPV_SYN_FB, c );
	}

struct SpvAna
	{
	const float * audio;      // [ch][n]
	flanhip_MF * out;         // [ch][n][N]
	const float2 * tab;       // [L]
	int64_t n, C, chains;     // frames, frames per chain, chains per channel
	int N, L, tiles;
	float sr, rL;             // rL = 1 / L when L is a power of two, else 0 (division)
	};

__device__ __forceinline__ int wrap_add( int i, int b, int L ) { i += b; return i >= L ? i - L : i; }

template<int B, bool LDS_TAB>
__global__ __launch_bounds__( 64 ) void k_spv_analyze( SpvAna p )
	{
	extern __shared__ float2 s_tab[];
	__shared__ float s_x[SPV_XB], s_xo[SPV_XB];
	const int lane = threadIdx.x;
	const int64_t blk = blockIdx.x;
	const int tile = int( blk % p.tiles );
	const int64_t chain = ( blk / p.tiles ) % p.chains;
	const int64_t c = blk / ( int64_t( p.tiles ) * p.chains );
	const int N = p.N, L = p.L;
	const float2 * T = p.tab;
	if constexpr( LDS_TAB )
		{
		for( int i = lane; i < L; i += 64 ) s_tab[i] = p.tab[i];
		__syncthreads();
		T = s_tab;
		}
	const float * x = p.audio + c * p.n;
	const int64_t f0 = chain * p.C;
	const int64_t f1 = std::min( f0 + p.C, p.n );
	const int64_t fs = std::max<int64_t>( f0 - 1, 0 );        // the halo frame (none for the channel's first chain)

	// bins: B owned, contiguous; one extra (lane 0: the bin below the tile, every other lane: the bin above it -- only lane 63's is used)
	const int lo = tile * 64 * B;
	int bin[B + 1];
	#pragma unroll
	for( int j = 0; j < B; ++j ) bin[j] = lo + lane * B + j;
	bin[B] = lane == 0 ? lo - 1 : lo + 64 * B;
	int bw[B + 1];                                             // the bin walked: out-of-range bins walk bin 0 (never read)
	#pragma unroll
	for( int j = 0; j <= B; ++j ) bw[j] = ( bin[j] >= 0 && bin[j] < N ) ? bin[j] : 0;

	// seed: S at frame fs - 1 = sum over j in [fs - L, fs) of x[j] T[(j b) mod L]
	float Sr[B + 1], Si[B + 1];
	int idx[B + 1];
	const int64_t j0 = std::max<int64_t>( fs - L, 0 );
	#pragma unroll
	for( int j = 0; j <= B; ++j ) { Sr[j] = 0.0f; Si[j] = 0.0f; idx[j] = int( ( j0 * int64_t( bw[j] ) ) % L ); }
	for( int64_t jb = j0; jb < fs; jb += SPV_XB )
		{
		__syncthreads();
		s_x[lane] = jb + lane < fs ? x[jb + lane] : 0.0f;
		__syncthreads();
		const int cnt = int( std::min<int64_t>( SPV_XB, fs - jb ) );
		for( int i = 0; i < cnt; ++i )
			{
			const float v = s_x[i];
			#pragma unroll
			for( int j = 0; j <= B; ++j )
				{
				const float2 t = T[idx[j]];
				Sr[j] = __builtin_fmaf( v, t.x, Sr[j] );
				Si[j] = __builtin_fmaf( v, t.y, Si[j] );
				idx[j] = wrap_add( idx[j], bw[j], L );
				}
			}
		}

	// per-bin constants of phase_vocoder (phase_vocoder.cpp:43-50 with SPVBuffer::bin_to_frequency = b sr / N)
	float bf[B], ex[B], prev[B];
	#pragma unroll
	for( int j = 0; j < B; ++j )
		{
		bf[j] = float( bw[j] ) * p.sr / float( N );
		ex[j] = bf[j] / p.sr * FLANHIP_PI2_F;
		prev[j] = 0.0f;
		}
	float2 tn[B + 1];
	#pragma unroll
	for( int j = 0; j <= B; ++j ) tn[j] = T[idx[j]];
	const bool pow2 = p.rL != 0.0f;
	const float Lf = float( L );

	for( int64_t fb = fs; fb < f1; fb += SPV_XB )
		{
		__syncthreads();
		{
		const int64_t f = fb + lane;
		s_x[lane] = f < f1 ? x[f] : 0.0f;
		s_xo[lane] = ( f < f1 && f - L >= 0 ) ? x[f - L] : 0.0f;
		}
		__syncthreads();
		const int cnt = int( std::min<int64_t>( SPV_XB, f1 - fb ) );
		for( int i = 0; i < cnt; ++i )
			{
			const int64_t f = fb + i;
			const float d = s_x[i] - s_xo[i];                             // AudioSPV.cpp:50
			float Fr[B + 1], Fi[B + 1];
			#pragma unroll
			for( int j = 0; j <= B; ++j )
				{
				// :57  S += d T[(f b) mod L]
				const float pr = d * tn[j].x, pi = d * tn[j].y;
				Sr[j] = Sr[j] + pr;
				Si[j] = Si[j] + pi;
				idx[j] = wrap_add( idx[j], bw[j], L );
				tn[j] = T[idx[j]];
				// :64-65  S conj( T[((f+1) b) mod L] )
				const float cr = tn[j].x, ci = -tn[j].y;
				Fr[j] = Sr[j] * cr - Si[j] * ci;
				Fi[j] = Sr[j] * ci + Si[j] * cr;
				}
			// neighbours across lanes: the last bin of the lane below, the first of the lane above; the tile's ends from the extra bin
			float lr = __shfl_up( Fr[B - 1], 1 ), li = __shfl_up( Fi[B - 1], 1 );
			float rr = __shfl_down( Fr[0], 1 ), ri = __shfl_down( Fi[0], 1 );
			const float er = __shfl( Fr[B], 63 ), ei = __shfl( Fi[B], 63 );
			if( lane == 0 ) { lr = Fr[B]; li = Fi[B]; }
			if( lane == 63 ) { rr = er; ri = ei; }
			const bool emit = f >= f0;
			flanhip_MF mf[B];
			#pragma unroll
			for( int j = 0; j < B; ++j )
				{
				const float Lr = j == 0 ? lr : Fr[j - 1], Li = j == 0 ? li : Fi[j - 1];
				const float Rr = j == B - 1 ? rr : Fr[j + 1], Ri = j == B - 1 ? ri : Fi[j + 1];
				// :70-90  0.25 ( (F + F) - (F[b-1] + F[b+1]) ) / L;  bin 0: F[b-1] + F[b+1] -> 2 Re F[1];  bin N-1: -> 2 Re F[N-2]
				const float ar = Fr[j] + Fr[j], ai = Fi[j] + Fi[j];
				float br, bi;
				if( bin[j] == 0 ) { br = Rr * 2.0f; bi = 0.0f; }
				else if( bin[j] == N - 1 ) { br = Lr * 2.0f; bi = 0.0f; }
				else { br = Lr + Rr; bi = Li + Ri; }
				float vr = 0.25f * ( ar - br ), vi = 0.25f * ( ai - bi );
				if( pow2 ) { vr = vr * p.rL; vi = vi * p.rL; }
				else { vr = vr / Lf; vi = vi / Lf; }
				// phase_vocoder.cpp:43-52, use_wrapping false (analysis rate == sample rate)
				const float ph = atan2_fast( vi, vr );
				const float m = magnitude_scaled( vr, vi );
				const float pd = ph - prev[j];
				prev[j] = ph;
				const float dp = pd - ex[j];
				const float df = div_pi2( dp * p.sr );
				mf[j].m = m;
				mf[j].f = bf[j] + df;
				}
			if( emit )
				{
				flanhip_MF * row = p.out + ( c * p.n + f ) * int64_t( N );
				const int b0 = bin[0];
				if( ( B % 2 == 0 ) && ( N % 2 == 0 ) && b0 + B <= N )
					{
					float4 * q = reinterpret_cast<float4*>( row + b0 );
					#pragma unroll
					for( int j = 0; j < B; j += 2 ) q[j / 2] = make_float4( mf[j].m, mf[j].f, mf[j + 1].m, mf[j + 1].f );
					}
				else
					{
					#pragma unroll
					for( int j = 0; j < B; ++j ) if( bin[j] < N ) row[bin[j]] = mf[j];
					}
				}
			}
		}
	}

struct SpvSyn
	{
	const flanhip_MF * spv;   // [ch][n][N]
	double * carry;           // [ch][chains][N]: chain sums, then carries
	double * peak;            // [ch][chains][N]: the highest prefix sum of each chain
	float * out;              // [ch][n]
	int64_t n, C, chains;
	int N;
	float ar;
	};

// phase_vocoder.cpp:57-59: phase += double( f / ar * pi2 ); if( phase > pi2 ) phase = fmod( phase, pi2 )
__device__ __forceinline__ double spv_advance( double ph, float f, float ar )
	{
	const float pd = f / ar * FLANHIP_PI2_F;
	ph = ph + double( pd );
	return ph < FLANHIP_FOLD_FAST_LIMIT ? fold_phase_fast( ph ) : fold_phase_any( ph );
	}

// What a chain does to the phase that enters it.  The reference folds only a phase above pi2, by the FLOAT pi2 (each fold moves the
// angle by 1.7e-7 rad), and never a negative one; which multiple of pi2 it holds is therefore part of its result, and so is the
// number of folds.  With U_i the chain's unfolded prefix sums, a phase p that enters has been folded floor( ( p + max_i U_i ) / pi2 )
// times by the chain's end if p + max_i U_i > pi2, and not at all otherwise: a chain is summed up by its total and its highest prefix
// sum, and the scan applies them to the true carry.  (Folding each chain's sum on its own, as if it started from 0, folds where the
// reference does not: a phase that wanders on both sides of 0, a repitched analysis for one, then sinks by one pi2 after another.)
// The unfolded sums are exact to well below the float( phase ) the cosine takes while they stay under 2^21 rad (ulp 4.7e-10).  Above --
// a chain held near 1e9 Hz, one MF of 1e20 Hz, where the reference's own addition rounds the running phase to whole radians, or a
// frequency that is not finite -- what comes out depends on the phase that went in: such a chain hands the scan SPV_REWALK instead of
// a total, and the scan walks its frames from the carry like the reference.  +inf is free for that: no other total reaches it.
#define SPV_SUM_LIMIT 0x1p21
#define SPV_REWALK __builtin_inf()

// one thread per (channel, chain, bin): the chain's unfolded total (or SPV_REWALK) and its highest prefix sum
__global__ __launch_bounds__( 256 ) void k_spv_chain_sums( SpvSyn p, int64_t ch )
	{
	const int64_t t = int64_t( blockIdx.x ) * blockDim.x + threadIdx.x;
	if( t >= ch * p.chains * p.N ) return;
	const int b = int( t % p.N );
	const int64_t chain = ( t / p.N ) % p.chains;
	const int64_t c = t / ( int64_t( p.N ) * p.chains );
	if( chain == p.chains - 1 ) return;                                   // the last chain's sum is nobody's carry
	const int64_t f0 = chain * p.C, f1 = std::min( f0 + p.C, p.n );
	const flanhip_MF * col = p.spv + ( c * p.n ) * int64_t( p.N ) + b;
	double u = 0.0, top = 0.0;
	bool exact = true;
	for( int64_t f = f0; f < f1; ++f )
		{
		const float pd = col[f * p.N].f / p.ar * FLANHIP_PI2_F;
		u = u + double( pd );
		exact = exact && __builtin_fabs( u ) < SPV_SUM_LIMIT;              // false for a NaN as well
		top = u > top ? u : top;
		}
	p.carry[t] = exact ? u : SPV_REWALK;
	p.peak[t] = top;
	}

// one thread per (channel, bin): carries in place, carry[0] = 0, carry[k+1] = carry[k] + sum[k] less the folds the reference made on the
// way, or chain k walked from carry[k]
__global__ __launch_bounds__( 256 ) void k_spv_scan( SpvSyn p, int64_t ch )
	{
	const int64_t t = int64_t( blockIdx.x ) * blockDim.x + threadIdx.x;
	if( t >= ch * p.N ) return;
	const int b = int( t % p.N );
	const int64_t c = t / p.N;
	double * col = p.carry + c * p.chains * p.N + b;
	const double * pk = p.peak + c * p.chains * p.N + b;
	// the loads do not depend on the carry: 16 of them in flight at a time, then the dependent adds (a 1-channel scan walks ~2000 chains)
	double carry = 0.0;
	for( int64_t k0 = 0; k0 < p.chains; k0 += 16 )
		{
		double s[16], top[16];
		#pragma unroll
		for( int i = 0; i < 16; ++i )
			{
			const bool have = k0 + i < p.chains - 1;                          // the last chain's sum is never written
			s[i] = have ? col[( k0 + i ) * p.N] : 0.0;
			top[i] = have ? pk[( k0 + i ) * p.N] : 0.0;
			}
		#pragma unroll
		for( int i = 0; i < 16; ++i )
			{
			if( k0 + i >= p.chains ) break;
			col[( k0 + i ) * p.N] = carry;
			if( s[i] == SPV_REWALK )
				{
				const flanhip_MF * mf = p.spv + ( c * p.n ) * int64_t( p.N ) + b;
				const int64_t f0 = ( k0 + i ) * p.C, f1 = std::min( f0 + p.C, p.n );
				for( int64_t f = f0; f < f1; ++f ) carry = spv_advance( carry, mf[f * p.N].f, p.ar );
				continue;
				}
			const double high = carry + top[i];
			double q = 0.0;
			if( high > FLANHIP_PI2_D )
				{
				q = __builtin_floor( high / FLANHIP_PI2_D );
				if( __builtin_fma( -q, FLANHIP_PI2_D, high ) < 0.0 ) q -= 1.0;
				}
			carry = __builtin_fma( -q, FLANHIP_PI2_D, carry + s[i] );
			}
		}
	}

// one block per (channel, chain); thread t owns bins t, t + 256, ...  K: bins per thread held in registers (0: any count, the running
// phases in the carry rows of the workspace, which the block owns)
template<int K>
__global__ __launch_bounds__( SPV_SYN_THREADS ) void k_spv_synthesize( SpvSyn p )
	{
	__shared__ float s_part[SPV_SYN_FB][SPV_SYN_THREADS + 1];
	__shared__ float s_seg[SPV_SYN_FB][SPV_SYN_THREADS / SPV_SYN_FB + 1];
	const int t = threadIdx.x;
	const int64_t chain = blockIdx.x % p.chains;
	const int64_t c = blockIdx.x / p.chains;
	const int N = p.N;
	double * carry = p.carry + ( c * p.chains + chain ) * int64_t( N );
	const int64_t f0 = chain * p.C, f1 = std::min( f0 + p.C, p.n );
	double ph[K > 0 ? K : 1];
	if constexpr( K > 0 )
		{
		#pragma unroll
		for( int k = 0; k < K; ++k ) { const int b = t + SPV_SYN_THREADS * k; ph[k] = b < N ? carry[b] : 0.0; }
		}
	for( int64_t fb = f0; fb < f1; fb += SPV_SYN_FB )
		{
		const int cnt = int( std::min<int64_t>( SPV_SYN_FB, f1 - fb ) );
		for( int i = 0; i < cnt; ++i )
			{
			const flanhip_MF * row = p.spv + ( c * p.n + fb + i ) * int64_t( N );
			float part = 0.0f;
			if constexpr( K > 0 )
				{
				#pragma unroll
				for( int k = 0; k < K; ++k )
					{
					const int b = t + SPV_SYN_THREADS * k;
					if( b < N )
						{
						const flanhip_MF mf = row[b];
						ph[k] = spv_advance( ph[k], mf.f, p.ar );
						const float fp = float( ph[k] );
						float s, co;
						if( __builtin_fabsf( fp ) < FLANHIP_SINCOS_FAST_LIMIT ) sincos_fast( fp, s, co );
						else { const float2 w = sincos_wide( fp ); co = w.y; }
						const float re = mf.m * co;                       // std::polar( m, float( phase ) ).real()
						part += ( b & 1 ) ? -re : re;                      // AudioSPV.cpp:138
						}
					}
				}
			else
				{
				for( int b = t; b < N; b += SPV_SYN_THREADS )
					{
					const flanhip_MF mf = row[b];
					const double q = spv_advance( carry[b], mf.f, p.ar );
					carry[b] = q;
					const float fp = float( q );
					float s, co;
					if( __builtin_fabsf( fp ) < FLANHIP_SINCOS_FAST_LIMIT ) sincos_fast( fp, s, co );
					else { const float2 w = sincos_wide( fp ); co = w.y; }
					const float re = mf.m * co;
					part += ( b & 1 ) ? -re : re;
					}
				}
			s_part[i][t] = part;
			}
		__syncthreads();
		{
		constexpr int SEG = SPV_SYN_THREADS / SPV_SYN_FB;                    // 8 segments of 32 partials per frame
		const int i = t % SPV_SYN_FB, sg = t / SPV_SYN_FB;
		float v = 0.0f;
		if( i < cnt ) for( int k = 0; k < SPV_SYN_THREADS / SEG; ++k ) v += s_part[i][sg * ( SPV_SYN_THREADS / SEG ) + k];
		s_seg[i][sg] = v;
		}
		__syncthreads();
		if( t < cnt )
			{
			float v = 0.0f;
			for( int k = 0; k < SPV_SYN_THREADS / SPV_SYN_FB; ++k ) v += s_seg[t][k];
			p.out[c * p.n + fb + t] = v * 2.0f;                               // AudioSPV.cpp:140
			}
		}
	}

__global__ __launch_bounds__( 256 ) void k_spv_modify_frequency_const( const flanhip_MF * in, int64_t count, float value, int multiply, flanhip_MF * out )
	{
	const int64_t stride = int64_t( gridDim.x ) * blockDim.x;
	for( int64_t i = int64_t( blockIdx.x ) * blockDim.x + threadIdx.x; i < count; i += stride )
		{
		flanhip_MF mf = in[i];
		mf.f = multiply ? mf.f * value : value;                             // SPV.cpp:33 with f = c, or :43 with f * c
		out[i] = mf;
		}
	}

template<int B>
int launch_ana_b( const SpvAna & p, int64_t blocks, hipStream_t s )
	{
	const size_t tab_bytes = sizeof( float2 ) * size_t( p.L );
	if( tab_bytes <= 64 * 1024 ) return launch_kernel( __func__, k_spv_analyze<B, true>, blocks, 64, tab_bytes, s, p );
	return launch_kernel( __func__, k_spv_analyze<B, false>, blocks, 64, 0, s, p );
	}

int spv_check( int64_t ch, int64_t n, int N, float sr )
	{
	FLANHIP_REQUIRE( ch > 0 && n > 0 && sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "bad sizes" );
	FLANHIP_REQUIRE( N >= 2, FLANHIP_ERR_UNSUPPORTED, "num_bins below 2 (the reference reads bin 1 of every frame)" );
	FLANHIP_REQUIRE( N <= ( 1 << 24 ), FLANHIP_ERR_UNSUPPORTED, "num_bins above 2^24" );
	return FLANHIP_OK;
	}

int launch_spv_analyze( const float * d_audio, int64_t ch, int64_t n, float sr, int N, flanhip_MF * d_out, hipStream_t s )
	{
	FLANHIP_REQUIRE( d_audio && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	if( int rc = spv_check( ch, n, N, sr ) ) return rc;
	if( int rc = require_device() ) return rc;
	SpvAna p;
	p.audio = d_audio; p.out = d_out;
	p.N = N; p.L = 2 * N; p.n = n; p.sr = sr;
	p.rL = is_pow2( p.L ) ? 1.0f / float( p.L ) : 0.0f;
	if( int rc = get_table( p.L, &p.tab ) ) return rc;
	const int B = spv_bins_per_lane( N );
	p.tiles = int( ( int64_t( N ) + 64 * B - 1 ) / ( 64 * B ) );
	p.C = spv_analysis_chain( ch, n, N, p.tiles );
	p.chains = ( n + p.C - 1 ) / p.C;
	const int64_t blocks = ch * p.chains * p.tiles;
	switch( B )
		{
		case 1: return launch_ana_b<1>( p, blocks, s );
		case 2: return launch_ana_b<2>( p, blocks, s );
		case 4: return launch_ana_b<4>( p, blocks, s );
		default: return launch_ana_b<8>( p, blocks, s );
		}
	}

size_t spv_ws_bytes( int64_t ch, int64_t n, int N )
	{
	const int64_t C = spv_synthesis_chain( ch, n );
	const int64_t chains = ( n + C - 1 ) / C;
	return 2 * sizeof( double ) * size_t( ch ) * size_t( chains ) * size_t( N );      // totals / carries, and peaks
	}

int launch_spv_synthesize( const flanhip_MF * d_spv, int64_t ch, int64_t n, int N, float sr, float * d_out, void * d_ws, hipStream_t s )
	{
	FLANHIP_REQUIRE( d_spv && d_out && d_ws, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	if( int rc = spv_check( ch, n, N, sr ) ) return rc;
	if( int rc = require_device() ) return rc;
	SpvSyn p;
	p.spv = d_spv; p.carry = ws_at<double>( d_ws, 0 ); p.out = d_out;
	p.n = n; p.N = N; p.ar = sr;
	p.C = spv_synthesis_chain( ch, n );
	p.chains = ( n + p.C - 1 ) / p.C;
	p.peak = p.carry + ch * p.chains * int64_t( N );
	const int64_t blocks = ch * p.chains;
	if( p.chains > 1 )
		{
		const int64_t th = ch * p.chains * N, tc = ch * N;
		if( int rc = launch_kernel( __func__, k_spv_chain_sums, ( th + 255 ) / 256, 256, 0, s, p, ch ) ) return rc;
		if( int rc = launch_kernel( __func__, k_spv_scan, ( tc + 255 ) / 256, 256, 0, s, p, ch ) ) return rc;
		}
	else FLANHIP_CHECK( hipMemsetAsync( d_ws, 0, sizeof( double ) * size_t( ch ) * N, s ) );
	const int K = ( N + SPV_SYN_THREADS - 1 ) / SPV_SYN_THREADS;
	auto go = [&]( auto kernel ) { return launch_kernel( "launch_spv_synthesize", kernel, blocks, SPV_SYN_THREADS, 0, s, p ); };
	if( K <= 1 ) return go( k_spv_synthesize<1> );
	if( K <= 2 ) return go( k_spv_synthesize<2> );
	if( K <= 4 ) return go( k_spv_synthesize<4> );
	if( K <= 8 ) return go( k_spv_synthesize<8> );
	if( K <= 16 ) return go( k_spv_synthesize<16> );
	return go( k_spv_synthesize<0> );
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

int flanhip_spv_twiddles( int num_bins, float * out )
	{
	FLANHIP_REQUIRE( out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_bins >= 2, FLANHIP_ERR_UNSUPPORTED, "num_bins below 2" );
	host_twiddles( 2 * num_bins, out );
	return FLANHIP_OK;
	}

void flanhip_spv_debug_chain_length( int frames )
	{
	t_spv_chain_len = frames > 0 ? frames : 0;
	}

int flanhip_spv_analyze_dev( const float * d_audio, int64_t ch, int64_t n, float sr, int num_bins, flanhip_MF * d_out, void * stream )
	{
	return launch_spv_analyze( d_audio, ch, n, sr, num_bins, d_out, (hipStream_t) stream );
	}

int flanhip_spv_analyze( const float * audio, int64_t ch, int64_t n, float sr, int num_bins, flanhip_MF * out, volatile int * cancel )
	{
	FLANHIP_REQUIRE( audio && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	if( int rc = spv_check( ch, n, num_bins, sr ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	const float * d_audio = nullptr; flanhip_MF * d_out = nullptr;
	if( int rc = call.in( audio, sizeof( float ) * size_t( ch ) * size_t( n ), &d_audio ) ) return rc;
	if( int rc = call.out( out, sizeof( flanhip_MF ) * size_t( ch ) * size_t( n ) * size_t( num_bins ), &d_out ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_spv_analyze( d_audio, ch, n, sr, num_bins, d_out, nullptr ) ) return rc;
	return call.finish();
	}

size_t flanhip_spv_synthesize_workspace_bytes( int64_t ch, int64_t n, int num_bins, float sr )
	{
	if( ch <= 0 || n <= 0 || num_bins < 2 || num_bins > ( 1 << 24 ) || !( sr > 0.0f ) ) return 0;
	return spv_ws_bytes( ch, n, num_bins );
	}

int flanhip_spv_synthesize_dev( const flanhip_MF * d_spv, int64_t ch, int64_t n, int num_bins, float sr, float * d_out, void * d_workspace, void * stream )
	{
	return launch_spv_synthesize( d_spv, ch, n, num_bins, sr, d_out, d_workspace, (hipStream_t) stream );
	}

int flanhip_spv_synthesize( const flanhip_MF * spv, int64_t ch, int64_t n, int num_bins, float sr, float * out, volatile int * cancel )
	{
	FLANHIP_REQUIRE( spv && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	if( int rc = spv_check( ch, n, num_bins, sr ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	const flanhip_MF * d_spv = nullptr; float * d_out = nullptr; void * d_ws = nullptr;
	if( int rc = call.in( spv, sizeof( flanhip_MF ) * size_t( ch ) * size_t( n ) * size_t( num_bins ), &d_spv ) ) return rc;
	if( int rc = call.out( out, sizeof( float ) * size_t( ch ) * size_t( n ), &d_out ) ) return rc;
	if( int rc = call.scratch( spv_ws_bytes( ch, n, num_bins ), &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_spv_synthesize( d_spv, ch, n, num_bins, sr, d_out, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

int flanhip_spv_modify_frequency_const_dev( const flanhip_MF * d_spv, int64_t ch, int64_t n, int num_bins, float value, int multiply,
	flanhip_MF * d_out, void * stream )
	{
	FLANHIP_REQUIRE( d_spv && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch > 0 && n > 0 && num_bins > 0, FLANHIP_ERR_INVALID_ARG, "bad sizes" );
	if( int rc = require_device() ) return rc;
	const int64_t count = ch * n * int64_t( num_bins );
	const int64_t blocks = std::min<int64_t>( ( count + 255 ) / 256, 8192 );
	return launch_kernel( __func__, k_spv_modify_frequency_const, blocks, 256, 0, (hipStream_t) stream, d_spv, count, value, multiply, d_out );
	}

} // extern "C"
