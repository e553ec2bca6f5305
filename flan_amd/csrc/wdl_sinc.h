// wdl_sinc.h -- WDL_Resampler's windowed-sinc mode (WDL/resample.cpp, SetMode( true, 0, true, TAPS )) as far as it does not depend on who
// feeds it, written ONCE: repitch.hip and wavetable.hip use it at 64 taps, spatial.hip (head_itd) at 32.  DESIGN.md section 4.13.
//
// A caller's host plan reproduces the resampler's state block by block and hands every block a ( filtpos, oversize, ideal ) table
// (wdl_table_shape) and a read position (wdl_hand_over).  On the device k_wdl_window leaves the Blackman-Harris factor of every table
// entry once per call, a workgroup builds its table in LDS (wdl_build_table), and every output sample is an independent sum of TAPS
// products (wdl_sample) over one continuous stream: TAPS / 2 - 1 zeros, the input, zeros (wdl_stream).
// Every sum runs in a fixed order, so two runs agree bit for bit.
#pragma once
#include "flanhip_internal.h"

#include <algorithm>
#include <vector>

namespace flanhip {

constexpr int WDL_OVERSIZE = 32;               // m_sincoversize (SetMode's default), the slices of a table that is not "ideal"
constexpr int WDL_MAX_OVERSIZE = 2 * WDL_OVERSIZE;             // an ideal table may have up to 2 x 32 slices (:1135)
constexpr int WDL_THREADS = 256;

template<int TAPS> struct WdlSinc              // TAPS: m_sincsize
	{
	static constexpr int PRELUDE = TAPS / 2 - 1;                 // zeros in front of the stream (:1226-1237)
	static constexpr int SLICE_STRIDE = TAPS + 1;                // LDS floats per table slice: lanes read tap i of DIFFERENT slices, the odd stride spreads them over the 64 banks
	static constexpr int TABLE_FLOATS = ( WDL_MAX_OVERSIZE + 1 ) * SLICE_STRIDE;
	static constexpr int WIN_SLOT = ( WDL_MAX_OVERSIZE + 1 ) * ( TAPS / 2 );     // doubles per oversize in the window-factor table (its largest half table)
	};

// BuildLowPass's choice of table (:1095-1141); it does not depend on the tap count
inline void wdl_table_shape( double rate_in, double rate_out, double ratio, double * filtpos, int * oversize, int * ideal )
	{
	*filtpos = ratio > 1.0 ? 1.0 / ( ratio * 1.03 ) : 1.0;                   // :1327-1328
	int want = WDL_OVERSIZE, ideal_interp = 0;
	if( ratio < 1.0 )
		{
		const double drat = rate_out / rate_in;
		const int irat = int( drat + 0.5 );
		if( irat > 1 && irat == drat ) ideal_interp = irat;
		}
	else
		{
		const int irat = int( ratio + 0.5 );
		if( ratio == irat ) ideal_interp = 1;
		}
	if( !ideal_interp && rate_in < 2147483648.0 && rate_out < 2147483648.0 )
		{
		const int in1 = int( rate_in ), out1 = int( rate_out );
		if( out1 > 0 && in1 > 0 && rate_in == double( in1 ) && rate_out == double( out1 ) )
			{
			int min_cd = out1 / ( 2 * want );
			if( min_cd < 1 ) min_cd = 1;
			int n1 = out1, n2 = in1;
			while( n2 >= min_cd ) { const int tmp = n1; n1 = n2; n2 = tmp % n2; }
			if( !n2 ) ideal_interp = out1 / n1;
			}
		}
	if( ideal_interp > 0 && ideal_interp <= want * 2 ) want = ideal_interp;
	*oversize = want;
	*ideal = ideal_interp == want;
	}

// ResampleOut's hand-over at the end of a block (:1558-1563), srcpos being where the block's chain of += ratio stopped and S the samples
// buffered: the whole samples the buffer drops (returned) and the fractional position the next block starts from
inline int64_t wdl_hand_over( double srcpos, int64_t S, int ideal, int oversize, double * fracpos )
	{
	const int64_t isrcpos = std::min( int64_t( srcpos ), S );                // :1558-1559
	*fracpos = srcpos - double( isrcpos );
	if( ideal ) *fracpos = std::floor( oversize * *fracpos + 0.5 ) / oversize;   // :1562-1563
	return isrcpos;
	}

// the same columns for a *_plan entry point: each array nullable, filled up to `capacity`; extra( i, block ) adds the caller's own
template<class Block, class Extra>
inline int64_t wdl_export_plan( const std::vector<Block> & blocks, int64_t num_blocks, int64_t capacity, int64_t * offsets, double * fracpos, double * ratio,
	double * filtpos, int32_t * oversize, int32_t * ideal, int64_t * first_out, Extra extra )
	{
	const int64_t fill = std::min<int64_t>( std::max<int64_t>( capacity, 0 ), num_blocks );
	for( int64_t i = 0; i < fill; ++i )
		{
		const Block & b = blocks[size_t( i )];
		if( offsets ) offsets[i] = b.offset;
		if( fracpos ) fracpos[i] = b.fracpos;
		if( ratio ) ratio[i] = b.ratio;
		if( filtpos ) filtpos[i] = b.filtpos;
		if( oversize ) oversize[i] = b.oversize;
		if( ideal ) ideal[i] = b.ideal;
		if( first_out ) first_out[i] = b.first_out;
		extra( i, b );
		}
	return num_blocks;
	}

// runs are consecutive blocks that read one table
template<class A, class B>
inline bool wdl_same_table( const A & a, const B & b ) { return a.oversize == b.oversize && a.ideal == b.ideal && a.filtpos == b.filtpos; }

// channels per workgroup: one where a run has work for every thread several times over, more where the table dominates
inline int wdl_channels_per_group( int64_t outputs, size_t num_runs, int64_t ch )
	{
	const int64_t per_run = std::max<int64_t>( outputs / std::max<int64_t>( int64_t( num_runs ), 1 ), 1 );
	return int( std::clamp<int64_t>( 512 / per_run, 1, ch ) );
	}

// the same and the channel groups a launch then has: its grid is runs x *groups
inline int wdl_channel_groups( int64_t outputs, size_t num_runs, int64_t ch, int64_t * groups )
	{
	const int cpw = wdl_channels_per_group( outputs, num_runs, ch );
	*groups = ( ch + cpw - 1 ) / cpw;
	return cpw;
	}

// the workspace of a call: the window factors, then the block records, then the run records
struct WdlLayout { size_t win_off, block_off, run_off, total; };
template<int TAPS>
inline WdlLayout wdl_layout( size_t block_bytes, int64_t num_blocks, size_t run_bytes, int64_t num_runs )
	{
	WdlLayout l;
	l.win_off = 0;
	l.block_off = sizeof( double ) * size_t( WDL_MAX_OVERSIZE ) * WdlSinc<TAPS>::WIN_SLOT;
	l.run_off = l.block_off + block_bytes * size_t( num_blocks );
	l.total = l.run_off + run_bytes * size_t( num_runs );
	return l;
	}

// sample `s` of the stream: `prelude` zeros, the n input frames, zeros
__device__ __forceinline__ float wdl_stream( const float * __restrict__ x, int64_t n, int64_t prelude, int64_t s )
	{
	const int64_t t = s - prelude;
	return ( t >= 0 && t < n ) ? x[t] : 0.0f;
	}
template<int TAPS>
__device__ __forceinline__ float wdl_stream( const float * __restrict__ x, int64_t n, int64_t s ) { return wdl_stream( x, n, WdlSinc<TAPS>::PRELUDE, s ); }

// The Blackman-Harris factor of every table entry, per oversize in use (bit blockIdx.x of `used`), in fp64: once per call.
// half table entry e is ( slice e / TAPS, tap e % TAPS ): every slice but the last has TAPS entries (:1164-1171)
template<int TAPS>
__global__ __launch_bounds__( WDL_THREADS ) void k_wdl_window( double * __restrict__ win, uint64_t used )
	{
	const int oversize = int( blockIdx.x ) + 1;
	if( !( ( used >> blockIdx.x ) & 1 ) ) return;
	const int half = ( TAPS / 2 ) * ( oversize + 1 );
	double * w = win + size_t( blockIdx.x ) * WdlSinc<TAPS>::WIN_SLOT;
	const double dwindowpos = 2.0 * 3.1415926535897932384626433832795 / double( TAPS );         // :1157
	for( int e = threadIdx.x; e < half; e += WDL_THREADS )
		{
		const double frac = double( e / TAPS ) / double( oversize );
		const double xfrac = frac + double( e % TAPS );
		const double windowpos = dwindowpos * xfrac;
		w[e] = 0.35875 - 0.48829 * cos( windowpos ) + 0.14128 * cos( 2 * windowpos ) - 0.01168 * cos( 3 * windowpos );   // :1185
		}
	}

// k_wdl_window for every oversize the runs use.  *d_win: where it leaves the factors.
template<int TAPS, class Run>
inline int wdl_window( const char * who, void * d_ws, const WdlLayout & l, const std::vector<Run> & runs, hipStream_t s, const double ** d_win )
	{
	*d_win = ws_at<double>( d_ws, l.win_off );
	uint64_t used = 0;
	for( const Run & r : runs ) used |= uint64_t( 1 ) << ( r.oversize - 1 );
	return launch_kernel( who, k_wdl_window<TAPS>, WDL_MAX_OVERSIZE, WDL_THREADS, 0, s, ws_at<double>( d_ws, l.win_off ), used );
	}

// The table of one ( filtpos, oversize ) in LDS (BuildLowPass :1157-1202), by a whole workgroup of WDL_THREADS: window x sinc in fp64
// rounded to float; filtpower in a fixed order (each thread its own entries in rising order, then a tree over the threads); the first
// half scaled and rounded again; the second half mirrors it.  w: k_wdl_window's row of this oversize.  s_tab float[TABLE_FLOATS], s_red
// double[WDL_THREADS].  The table is whole after the caller's next barrier.
template<int TAPS>
__device__ __forceinline__ void wdl_build_table( float * s_tab, double * s_red, const double * w, int oversize, double filtpos )
	{
	constexpr int SLICE_STRIDE = WdlSinc<TAPS>::SLICE_STRIDE;
	const int lane = threadIdx.x;
	const int half = ( TAPS / 2 ) * ( oversize + 1 );
	const double dsincpos = 3.1415926535897932384626433832795 * filtpos;
	double power = 0.0;
	for( int e = lane; e < half; e += WDL_THREADS )
		{
		const int slice = e / TAPS, tap = e % TAPS;
		float c = 1.0f;                                                          // the centre tap of slice 0 (:1173-1177)
		if( e != TAPS / 2 )
			{
			const double xfrac = double( slice ) / double( oversize ) + double( tap );
			const double sincpos = dsincpos * ( xfrac - double( TAPS / 2 ) );
			const double val = w[e] * sin( sincpos ) / sincpos;
			power += slice ? val * 2 : val;
			c = float( val );
			}
		s_tab[slice * SLICE_STRIDE + tap] = c;
		}
	s_red[lane] = power;
	__syncthreads();
	for( int off = WDL_THREADS / 2; off > 0; off >>= 1 )
		{
		if( lane < off ) s_red[lane] = s_red[lane] + s_red[lane + off];
		__syncthreads();
		}
	const double scale = double( oversize ) / ( s_red[0] + 1.0 );            // :1193
	for( int e = lane; e < half; e += WDL_THREADS )
		{
		const int at = ( e / TAPS ) * SLICE_STRIDE + e % TAPS;
		const float c = float( double( s_tab[at] ) * scale );
		s_tab[at] = c;
		const int m = 2 * half - 1 - e;                                          // :1202
		s_tab[( m / TAPS ) * SLICE_STRIDE + m % TAPS] = c;
		}
	}

// TAPS taps: float products (each rounded), added into fp64 in tap order (the SincSample templates, :106-257, with float samples and
// coefficients).  LDS_IN: the taps are in_lds[0 ... TAPS), else stream samples s0 ... of the row x
template<int TAPS, bool LDS_IN>
__device__ __forceinline__ void wdl_taps2( const float * f1, const float * f2, const float * in_lds, const float * __restrict__ x, int64_t n, int64_t s0,
	double * sum, double * sum2 )
	{
	double a = 0.0, b = 0.0;
	#pragma unroll 8
	for( int i = 0; i < TAPS; ++i )
		{
		const float v = LDS_IN ? in_lds[i] : wdl_stream<TAPS>( x, n, s0 + i );
		a += double( __fmul_rn( f1[i], v ) );
		b += double( __fmul_rn( f2[i], v ) );
		}
	*sum = a; *sum2 = b;
	}

template<int TAPS, bool LDS_IN>
__device__ __forceinline__ double wdl_taps1( const float * f2, const float * in_lds, const float * __restrict__ x, int64_t n, int64_t s0 )
	{
	double b = 0.0;
	#pragma unroll 8
	for( int i = 0; i < TAPS; ++i )
		{
		const float v = LDS_IN ? in_lds[i] : wdl_stream<TAPS>( x, n, s0 + i );
		b += double( __fmul_rn( f2[i], v ) );
		}
	return b;
	}

// One output sample: srcpos is its read position relative to stream index `offset` (a block's).  The taps come from the staged window
// s_in (stream samples win_start ... win_start + win_len) where it holds all of them, else from the row x of n frames.
template<int TAPS>
__device__ __forceinline__ float wdl_sample( const float * s_tab, const float * s_in, int64_t win_start, int win_len, const float * x, int64_t n,
	int64_t offset, double srcpos, int oversize, int ideal )
	{
	constexpr int SLICE_STRIDE = WdlSinc<TAPS>::SLICE_STRIDE;
	const int64_t ipos = int64_t( srcpos );
	const double frac = srcpos - double( ipos );
	const int64_t s0 = offset + ipos;                                            // stream index of tap 0
	const int64_t rel = s0 - win_start;
	const bool staged = rel >= 0 && rel + TAPS <= int64_t( win_len );
	if( ideal )
		{
		int ifpos = int( frac * oversize + 0.5 );                                // SincSample1N (:184-200)
		ifpos = ifpos < 0 ? 0 : ifpos > oversize ? oversize : ifpos;
		const float * f2 = s_tab + ( oversize - ifpos ) * SLICE_STRIDE;
		const double sum2 = staged ? wdl_taps1<TAPS, true>( f2, s_in + rel, x, n, s0 ) : wdl_taps1<TAPS, false>( f2, s_in, x, n, s0 );
		return float( sum2 );
		}
	double fr = frac * oversize;                                                 // SincSample1 (:160-182)
	int ifpos = int( fr );
	ifpos = ifpos < 0 ? 0 : ifpos > oversize - 1 ? oversize - 1 : ifpos;
	fr -= ifpos;
	const float * f2 = s_tab + ( oversize - ifpos ) * SLICE_STRIDE;
	const float * f1 = f2 - SLICE_STRIDE;
	double sum, sum2;
	if( staged ) wdl_taps2<TAPS, true>( f1, f2, s_in + rel, x, n, s0, &sum, &sum2 );
	else wdl_taps2<TAPS, false>( f1, f2, s_in, x, n, s0, &sum, &sum2 );
	return float( __dadd_rn( __dmul_rn( sum, fr ), __dmul_rn( sum2, 1.0 - fr ) ) );
	}

} // namespace flanhip
